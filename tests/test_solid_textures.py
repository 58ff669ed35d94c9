"""UVW textures: PetalTexture, LeafTexture and FlowerCenterTexture (csrc/mr_solid_body.h; mr_texture_lookup3 and mr_hit_surface on a
scene whose table holds one, both kernels of csrc/mr_procedural.hip).

The oracle has no textures and the reference's Texture.cpp needs GLUT, so the three lookup3D bodies are parity unpinned, like
stone's: this file restates them in numpy from the reference's lines (Texture.cpp:447-505, Texture.h:230-250,261-276),
importing nothing from the product.  The noise underneath is pinned already (tests/test_procedural.py, whose restatements of
the two noises, of StemTexture and of powf through glibc are imported rather than copied); the whole-number rule of
mr_solid_body.h is a wrapper of this file's own around them.  acos is numpy's double arccos rounded to float, which is what
mm_acosf is tested to be (tests/test_path_rays.py)."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

from test_procedural import (F, D, NONE, MISS, N_BATCH, PI, FLOOR_LIGHT, Traced, _cuda, _floor_rays, _host_scene, _stone_floor, dot3,
                             generate_noise, libm_powf, normalised, perlin, std_max, std_min, stem_lookup, worley2)

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import kernel_budget  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
assert generate_noise and worley2                                        # (used through stem_lookup; named by the module's contract)


# ---------------------------------------------------------------------------------------------------------------------------
# restatements (float32 numpy, the reference's order of operations)
# ---------------------------------------------------------------------------------------------------------------------------
def whole(c):
    return np.isfinite(c) & (c == np.floor(c))


def perlin_whole(x, y, z):
    """PerlinNoise::noise under the whole-number rule: (noise, undefined).  All coordinates whole: +-0 in the reference whatever
    int(floor()) yields, 0 here and not undefined.  Otherwise a coordinate that is NaN or reaches 2^30: undefined, 0."""
    x, y, z = (np.asarray(a, F) for a in (x, y, z))
    every = whole(x) & whole(y) & whole(z)
    with np.errstate(invalid="ignore"):
        inside = (np.abs(x) < F(2.0 ** 30)) & (np.abs(y) < F(2.0 ** 30)) & (np.abs(z) < F(2.0 ** 30))
    undefined = ~every & ~inside
    go = ~every & inside
    out = np.zeros(x.shape, F)
    out[go] = perlin(x[go], y[go], z[go])
    return out, undefined


def generate_noise_whole(x, y, initial_frequency, frequency_increase, amplitude_falloff, iterations):
    """generateNoise (Texture.h:20-37) with z = 0 over perlin_whole: (value, undefined in some octave)"""
    x, y = np.asarray(x, F), np.asarray(y, F)
    amplitude, frequency = F(1), F(initial_frequency)
    value, max_val = np.zeros(x.shape, F), F(0)
    undefined = np.zeros(x.shape, bool)
    with np.errstate(all="ignore"):
        for _ in range(iterations):
            nz, bad = perlin_whole((x * frequency).astype(F), (y * frequency).astype(F), np.zeros(x.shape, F) * frequency)
            undefined |= bad
            value = (value + amplitude * nz).astype(F)
            max_val = F(max_val + amplitude)
            frequency = F(frequency * F(frequency_increase))
            amplitude = F(amplitude * F(amplitude_falloff))
        return (value / max_val).astype(F), undefined


def acos_f(t):
    with np.errstate(invalid="ignore"):
        return np.arccos(np.asarray(t, F).astype(D)).astype(F)


def petal_coords(P, pivot, radius):
    """Texture.cpp:465-492: (u, v, dist) [n, 3].  position.normalize() works in place (Vector3.h:205-208): phi, theta and the
    side test read the unit vector; the dot products are formed as Vector3.h:242-246 forms them, zeros included."""
    P = np.asarray(P, F)
    with np.errstate(all="ignore"):
        p = (P - np.asarray(pivot, F)[None, :]).astype(F)
        length = np.sqrt(dot3(p, p)).astype(F)
        dist = (length / F(radius)).astype(F)
        p = (p * (F(1) / length).astype(F)[:, None]).astype(F)
        px, py, pz = p[:, 0], p[:, 1], p[:, 2]
        zero, one = F(0), F(1)
        phi = acos_f(-(((zero * px + one * py).astype(F) + zero * pz).astype(F)))
        v = (phi / PI).astype(F)
        theta = (acos_f(((px * one + py * zero).astype(F) + pz * zero).astype(F)) / F(F(2) * PI)).astype(F)
        side = ((zero * px + zero * py).astype(F) + F(-1) * pz).astype(F)
        u = np.where(side > 0, theta, (one - theta).astype(F)).astype(F)
    return np.stack([u, v, dist], 1)


def petal_turb(t):
    with np.errstate(all="ignore"):
        return std_min((libm_powf((t / F(0.1)).astype(F), F(0.85)) * F(1.5)).astype(F), F(1))


def petal_colour(coords):
    """Texture.cpp:457-463,472-474,496-502 from (u, v, dist): (rgb [n, 3], undefined [n])"""
    u, v, dist = (np.asarray(coords, F)[:, k] for k in range(3))
    t_high, bad_high = generate_noise_whole(u, (v.astype(D) * 0.25).astype(F), 4, 2, 0.9, 10)
    t_low, bad_low = generate_noise_whole(u, v, 4, 3, 0.9, 25)
    high, low = petal_turb(np.abs(t_high)), petal_turb(np.abs(t_low))
    base_highlight, tip_highlight = (0.2, 0, 0.8), (0.8, 0.5, 1)
    base_depression, tip_depression = (0.2, 0.0, 0.5), (0.3, 0.15, 0.75)
    base_color, tip_color = (0.1, 0.0, 0.6), (0.6, 0.3, 1.0)
    near = (F(1) - dist).astype(F)
    out = []
    with np.errstate(all="ignore"):
        for c in range(3):
            mix = lambda a, b: ((near * F(a[c])).astype(F) + (dist * F(b[c])).astype(F)).astype(F)      # noqa: E731
            diffuse, highlight, depression = mix(base_color, tip_color), mix(base_highlight, tip_highlight), mix(base_depression, tip_depression)
            first = (((diffuse * high).astype(F) + (highlight * (F(1) - high).astype(F)).astype(F)).astype(F) * F(0.5)).astype(F)
            second = (((diffuse * low).astype(F) + (depression * (F(1) - low).astype(F)).astype(F)).astype(F) * F(0.5)).astype(F)
            out.append((first + second).astype(F))
    return np.stack(out, 1), bad_high | bad_low


def flower_centre_lookup(P, pivot, radius):
    """FlowerCenterTexture::lookup3D (Texture.h:261-276)"""
    P = np.asarray(P, F)
    with np.errstate(all="ignore"):
        d = (P - np.asarray(pivot, F)[None, :]).astype(F)
        dist = np.sqrt(dot3(d, d)).astype(F)
        fraction = std_max(std_min(libm_powf((dist / F(radius)).astype(F), F(30)), F(1)), F(0))
        rest = (F(1) - fraction).astype(F)
        red = std_min(((rest * F(0.31)).astype(F) + (fraction * F(0.92)).astype(F)).astype(F), F(1))
        green = std_min(((rest * F(0.18)).astype(F) + (fraction * F(0.71)).astype(F)).astype(F), F(1))
    return np.stack([red, green, np.full(len(P), F(0.1), F)], 1)


def same_bits(a, b):
    """bit-equal, a NaN equal to a NaN"""
    a, b = np.asarray(a, F), np.asarray(b, F)
    nan = np.isnan(a)
    return a.shape == b.shape and np.array_equal(nan, np.isnan(b)) and np.array_equal(a[~nan].view(np.uint32), b[~nan].view(np.uint32))


# ---------------------------------------------------------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------------------------------------------------------
DIFFUSE = ((1, 1, 1), (0, 0, 0), (0, 0, 0), 20.0, 1.0)
SHINY = ((1, 1, 1), (0.25, 0, 0), (0, 0.5, 0), 20.0, 1.5)
UVW_TABLE = [dict(petal=((0.25, -0.5, 0.0), 2.5)), dict(leaf=30.0), dict(flower_center=((-0.1, -0.35, 0.0), 1.1))]


def test_set_textures_accepts_the_uvw_kinds_on_a_host_only_scene(miro):
    from miro_amd import binding
    assert (binding.MR_TEX_PETAL, binding.MR_TEX_LEAF, binding.MR_TEX_FLOWER_CENTER) == (4, 5, 6)
    s = _host_scene(miro)
    s.set_materials([DIFFUSE, SHINY], [0, 1])
    for k, tex in enumerate(UVW_TABLE):
        s.set_textures([tex], [0, 0])                                    # a UVW texture may sit on a specular, refractive material
        assert s.procedural, k
        s.set_textures([])
        assert not s.procedural
        s.set_materials([DIFFUSE, SHINY], [0, 1])
    s.set_textures(UVW_TABLE + [dict(stone=3.0)], [3, 0])
    assert s.procedural


def test_set_textures_refuses_bad_uvw_textures_and_keeps_the_earlier_table(miro):
    from miro_amd import binding
    s = _host_scene(miro)
    L = miro.lib()
    s.set_materials([DIFFUSE, SHINY], [0, 1])
    s.set_textures([dict(color1=(1, 1, 1), color2=(0, 0, 0), scale=2.0)], [0, NONE])

    def table_still_there():
        with pytest.raises(miro.MiroError) as e:
            s.set_materials([DIFFUSE, SHINY], [0, 1])
        return e.value.status == -5

    def desc(kind, pivot=(0.0, 0.0, 0.0), radius=1.0, scale=1.0, reserved=0):
        d = binding.TextureDesc()
        d.kind, d.scale = kind, scale
        d.color1[:] = pivot
        d.color2[0] = radius
        d.reserved[2] = reserved
        return d

    def refused(d):
        st = L.mr_scene_set_textures(s.h, (binding.TextureDesc * 1)(d), 1, binding._u32p(np.array([0, NONE], np.uint32)))
        msg = L.mr_last_error()
        return st == -1 and table_still_there(), msg

    for kind in (binding.MR_TEX_PETAL, binding.MR_TEX_FLOWER_CENTER):
        for radius in (0.0, -1.0, np.nan, np.inf):
            ok, msg = refused(desc(kind, radius=radius))
            assert ok and b"radius" in msg, (kind, radius, msg)
        for pivot in ((np.nan, 0, 0), (0, np.inf, 0), (0, 0, -np.inf)):
            assert refused(desc(kind, pivot=pivot))[0], (kind, pivot)
        assert refused(desc(kind, scale=np.nan))[0]                      # a field the lookup never reads is checked all the same
        assert refused(desc(kind, reserved=1))[0]
    for bad in (desc(binding.MR_TEX_LEAF, scale=np.nan), desc(binding.MR_TEX_LEAF, scale=np.inf), desc(binding.MR_TEX_LEAF, pivot=(np.nan, 0, 0)),
                desc(binding.MR_TEX_LEAF, radius=np.nan)):
        assert refused(bad)[0]
    ok, msg = refused(desc(7))                                           # kind 7 stays unknown
    assert ok and b"unknown kind" in msg
    for good in (desc(binding.MR_TEX_LEAF, radius=0.0), desc(binding.MR_TEX_PETAL, radius=7.0), desc(binding.MR_TEX_FLOWER_CENTER, radius=1.1)):
        assert L.mr_scene_set_textures(s.h, (binding.TextureDesc * 1)(good), 1, binding._u32p(np.array([0, 0], np.uint32))) == 0


def test_texture_lookup3_is_exported_and_declared(miro):
    src = open(os.path.join(ROOT, "include", "miro_hip.h")).read()
    L = miro.lib()
    assert hasattr(L, "mr_texture_lookup3") and "mr_texture_lookup3" in miro.EXPORTED_SYMBOLS
    assert re.search(r"\bmr_status\s+mr_texture_lookup3\s*\(", src)
    assert re.search(r"MR_TEX_PETAL = 4, MR_TEX_LEAF = 5, MR_TEX_FLOWER_CENTER = 6", src)
    assert len(miro.EXPORTED_SYMBOLS) == len(set(miro.EXPORTED_SYMBOLS)) == 69
    s = _host_scene(miro)                                                # no device: MR_ERR_STATE, never a CPU path
    dummy = C.c_void_p(16)
    assert L.mr_texture_lookup3(s.h, 0, dummy, 4, dummy, None, None, None) == -5


def test_perlin_is_zero_on_whole_numbers():
    """The claim under the whole-number rule: the restated PerlinNoise::noise (pinned to the reference's own Perlin.cpp by
    tests/test_procedural.py) is exactly +-0 on whole-number coordinates -- 20 000 seeded triples up to 2^29, z = 0 and not."""
    rng = np.random.default_rng(23)
    mag = 2.0 ** rng.uniform(0, 29, (20000, 3))
    xyz = (np.floor(mag) * rng.choice([-1.0, 1.0], (20000, 3))).astype(F)
    xyz[::2, 2] = 0
    xyz[:3] = [[0, 0, 0], [2.0 ** 29, -2.0 ** 29, 0], [255, 256, 257]]
    assert (xyz == np.floor(xyz)).all() and np.abs(xyz).max() == 2.0 ** 29 and (np.abs(xyz) >= 2.0 ** 23).sum() > 5000
    assert (perlin(xyz[:, 0], xyz[:, 1], xyz[:, 2]) == 0).all()
    got, undefined = perlin_whole(F([3e12, 2.0 ** 31, np.nan, 2.0 ** 30, 0.5]), F([1e13, -2.0 ** 40, 1.0, 0.5, 0.25]), np.zeros(5, F))
    assert undefined.tolist() == [False, False, True, True, False] and (got[:4] == 0).all() and got[4] == perlin(F(0.5), F(0.25), F(0))


def test_few_petal_lookups_meet_an_undefined_octave():
    """PetalTexture's 25-octave turbulence on 200 000 seeded (u, v) in [0, 1)^2: the share of lookups with an octave that has a
    coordinate >= 2^30 and another that is not whole is below 1 % (measured: 0.34 %), where the bare 2^30 rule of mr_noise.h
    would count nearly all of them; the 10-octave call (last frequency 2 048) meets none."""
    rng = np.random.default_rng(29)
    uv = rng.random((200000, 2)).astype(F)
    _, undefined = generate_noise_whole(uv[:, 0], uv[:, 1], 4, 3, 0.9, 25)
    _, undefined10 = generate_noise_whole(uv[:, 0], (uv[:, 1].astype(D) * 0.25).astype(F), 4, 2, 0.9, 10)
    last = F(4) * F(3) ** 24
    print("undefined: %d of %d = %.3f %%; bare rule: %.1f %%" % (undefined.sum(), len(uv), 100.0 * undefined.mean(),
                                                                  100.0 * ((uv * last) >= 2.0 ** 30).any(axis=1).mean()))
    assert 0 < undefined.mean() < 0.01 and not undefined10.any()
    assert ((uv * last) >= 2.0 ** 30).any(axis=1).mean() > 0.99


def test_solid_kernels_stay_inside_the_verified_envelope():
    """The kernels that serve the UVW kinds, both in mr_procedural.hip (remarks in build/mr_procedural.remarks.txt) since the
    surface pass became one kernel: texture_lookup3_kernel and hit_surface_kernel, exactly one of each; no dynamic stack, no
    scratch; no more spilled VGPRs and no fewer waves per SIMD than BOTH its own record
    (tests/golden/kernel_budget_procedural.json, written by tools/kernel_budget.py --write-unit mr_procedural from the build
    whose GPU run of this file was green) AND the worst value among the kernels of tests/golden/kernel_budget.json.  The floors
    are those of the records the two had in the unit of their own: 8 waves per SIMD for the lookup, 6 for the surface pass."""
    unit = kernel_budget.unit_kernels("mr_procedural")
    cur = {}
    for word, waves in (("hit_surface_kernel", 6), ("texture_lookup3_kernel", 8)):
        name = [k for k in unit if word in k]
        assert len(name) == 1, word
        cur[name[0]] = unit[name[0]]
        assert cur[name[0]]["scratch_bytes_per_lane"] == 0 and cur[name[0]]["vgprs_spilled"] == 0, (name, cur[name[0]])
        assert cur[name[0]]["waves_per_simd"] >= waves, (name, cur[name[0]])
    kernel_budget.assert_inside_envelope(cur, "kernel_budget_procedural.json", also_main=True)


# ---------------------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------------------
PIVOTS = [((0.25, -0.5, 0.0), 2.5), ((-0.125, 0.375, 0.75), 1.75)]      # dyadic: pivot + offset and |offset| = radius are exact
N_POINTS = 32 * 256 + 3                                                  # 32 workgroups plus a 3-lane tail


def _lookup3(scene, texture, P, coords=True):
    import torch
    n = len(P)
    rgb = torch.full((n, 3), 7.0, dtype=torch.float32, device="cuda")
    crd = torch.full((n, 3), 7.0, dtype=torch.float32, device="cuda") if coords else None
    counts = torch.zeros(1, dtype=torch.int64, device="cuda")
    scene.texture_lookup3(texture, P if isinstance(P, torch.Tensor) else _cuda(np.asarray(P, F)), n, rgb, d_coords=crd, d_counts=counts)
    torch.cuda.synchronize()
    return rgb.cpu().numpy(), (crd.cpu().numpy() if coords else None), int(counts.item())


def petal_points(pivot, radius, n=N_POINTS, seed=31):
    """seeded points in a ball of 1.5 x radius round the pivot, then the traps"""
    rng = np.random.default_rng(seed)
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1)[:, None]
    P = (np.asarray(pivot, D)[None, :] + d * (1.5 * radius * rng.random(n) ** (1 / 3))[:, None]).astype(F)
    pv = np.asarray(pivot, F)
    traps = []
    for t in (0.5, 1.0, radius, 3.0):                                    # the +-y axis through the pivot
        traps += [pv + F([0, t, 0]), pv - F([0, t, 0])]
    traps += [F([1.0, 0.5, 0.0]), F([1.0, 0.5, -0.0]), F([-0.75, -1.0, 0.0]), F([-0.75, -1.0, -0.0]),          # z = 0 and z = -0
              pv + F([0.5, 0.25, 0]) * F([1, 1, 0]), pv.copy()]                                                # z = the pivot's; P == pivot
    traps += [pv + F([radius, 0, 0]), pv - F([radius, 0, 0]), pv + F([0, 0, radius]), pv - F([0, 0, radius]),  # distance exactly radius
              pv + F([0.6 * radius, 0.8 * radius, 0])]
    traps += [F([np.nan, 0, 0]), F([0, np.nan, 0]), F([0, 0, np.nan]), F([np.inf, 0, 0]), F([3e38, 3e38, -3e38])]
    for a in np.linspace(0.001, 0.012, 48):                              # close to the -y axis: v small while u * 4 * 3^18 passes 2^30
        traps.append(pv + F([radius * np.sin(a), -radius * np.cos(a), -0.01 * a]))
    for a in np.linspace(0.002, 0.03, 48):                               # close to the +x axis on the side z < 0: u small
        traps.append(pv + F([np.cos(a), 0.001, -np.sin(a)]))
    traps = np.array(traps, F)
    P[-len(traps):] = traps
    return P, len(traps)


@pytest.fixture(scope="module")
def board(miro):
    """a scene that only carries texture tables for mr_texture_lookup3: two triangles on the device"""
    s = miro.Scene(0)
    s.add_triangle([0, 0, 0, 1, 0, 0, 0, 1, 0], [0, 0, 1] * 3)
    s.add_triangle([0, 0, 1, 1, 0, 1, 0, 1, 1], [0, 0, 1] * 3)
    s.build(4)
    s.set_materials([DIFFUSE, SHINY], [0, 1])
    return s


@pytest.fixture(scope="module")
def petal_runs(miro, board):
    """mr_texture_lookup3 of two petal textures, each on its own point set: shared by the coordinate and the colour test"""
    board.set_textures([dict(petal=pv) for pv in PIVOTS], [0, 1])
    runs = []
    for k, (pivot, radius) in enumerate(PIVOTS):
        P, n_traps = petal_points(pivot, radius, seed=31 + k)
        rgb, crd, undefined = _lookup3(board, k, P)
        rgb_only, none, undefined_again = _lookup3(board, k, P, coords=False)            # d_coords = NULL
        assert none is None and same_bits(rgb, rgb_only) and undefined == undefined_again
        runs.append((pivot, radius, P, n_traps, rgb, crd, undefined))
    board.set_textures([])
    return runs


@pytest.mark.gpu
def test_petal_coordinates_are_bit_equal(petal_runs):
    """d_coords of mr_texture_lookup3 -- (u, v, dist) of Texture.cpp:465-492 -- against the restatement: bit for bit on seeded
    points in a ball of 1.5 x radius round a non-zero pivot and on the traps (the +-y axis through the pivot, z = +-0, P == pivot,
    distance exactly radius, NaN and infinite positions: NaN equal as NaN)."""
    for pivot, radius, P, n_traps, _, crd, _ in petal_runs:
        want = petal_coords(P, pivot, radius)
        differ = ~((crd.view(np.uint32) == want.view(np.uint32)) | (np.isnan(crd) & np.isnan(want))).all(axis=1)
        print("petal pivot %s radius %g: %d points (%d traps), rows that differ %d, NaN rows %d, u in [%.3f, %.3f], v in [%.3f, %.3f]" % (
            pivot, radius, len(P), n_traps, differ.sum(), np.isnan(want).any(axis=1).sum(), np.nanmin(want[:, 0]), np.nanmax(want[:, 0]),
            np.nanmin(want[:, 1]), np.nanmax(want[:, 1])))
        for k in np.nonzero(differ)[0][:8]:
            print("  P %s: got %s want %s" % (P[k].tolist(), [float(x).hex() for x in crd[k]], [float(x).hex() for x in want[k]]))
        assert same_bits(crd, want)
        on_pivot = (P == np.asarray(pivot, F)[None, :]).all(axis=1)
        assert on_pivot.sum() == 1 and np.isnan(want[on_pivot][0, :2]).all() and want[on_pivot][0, 2] == 0
        assert (want[:, 2] == 1).sum() >= 5 and np.isnan(want).any(axis=1).sum() >= 5
        ok = ~np.isnan(want).any(axis=1)
        assert want[ok, 0].min() < 0.01 and want[ok, 0].max() > 0.99 and want[ok, 1].min() < 0.01 and want[ok, 1].max() == 1


@pytest.mark.gpu
def test_petal_colour_from_the_devices_own_coordinates(petal_runs):
    """The restated colour, fed the device's (u, v, dist), lies within 3e-7 of d_rgb on every point, none left out, and the
    undefined count is the restatement's.  Where 3e-7 comes from: the only terms the two do not share are the two powf, at most
    1 ulp apart on [0, 1] (6e-8) -- each scaled by 1.5 and by half a colour difference below 0.7.  Why from the device's own
    coordinates: one ulp in u moves octaves 8 to 13 of the noise by whole cells, so the colour from P against a libm acosf
    would test acosf, not the kernel.  Largest difference measured on an MI355X: see DESIGN section 0."""
    for pivot, radius, P, _, rgb, crd, undefined in petal_runs:
        want, bad = petal_colour(crd)
        with np.errstate(invalid="ignore"):
            err = np.abs(rgb.astype(D) - want.astype(D))
        print("petal pivot %s: colour max abs err %.3g, undefined %d (restated %d) of %d, colour range [%.3f, %.3f], std %.3f" % (
            pivot, np.nanmax(err), undefined, bad.sum(), len(P), np.nanmin(want), np.nanmax(want), np.nanstd(want)))
        assert np.array_equal(np.isnan(rgb), np.isnan(want))
        assert not (np.nan_to_num(err) > 3e-7).any()
        assert undefined == bad.sum() and 0 < undefined < len(P) // 20
        assert np.nanstd(want) > 0.05


@pytest.mark.gpu
@pytest.mark.parametrize("scale", [1.0, 30.0])
def test_leaf_lookup_is_bit_equal(board, scale):
    """LeafTexture::lookup3D is StemTexture::lookup2D's body at (P.x, P.y) (Texture.h:230-250): bit-equal to the stem restatement,
    whatever P.z is; d_coords is not written."""
    rng = np.random.default_rng(37)
    P = rng.uniform(-3, 3, (N_BATCH, 3)).astype(F)
    P[:4] = [[0, 0, 0], [0.3, -1.7, 5.0], [-0.5, -0.5, -0.0], [1, 1, np.nan]]
    board.set_textures([dict(leaf=scale)], [0, NONE])
    got, crd, undefined = _lookup3(board, 0, P)
    board.set_textures([])
    assert got.tobytes() == stem_lookup(P[:, :2], scale).tobytes() and undefined == 0
    assert (crd == 7.0).all() and got[:, 1].std() > 0.01


@pytest.mark.gpu
def test_flower_centre_against_the_restatement(board):
    """FlowerCenterTexture::lookup3D against the restatement, whose powf is glibc's: within 2e-7 (one powf ulp on [0, 1] times
    the 0.61 span of red, and the roundings of the blend).  Points inside, on and beyond the radius, and P == pivot."""
    pivot, radius = (-0.125, -0.375, 0.5), 1.25
    rng = np.random.default_rng(41)
    d = rng.normal(size=(N_BATCH, 3))
    d /= np.linalg.norm(d, axis=1)[:, None]
    r = np.concatenate([rng.uniform(0, 0.8, N_BATCH // 4), rng.uniform(0.8, 1.05, N_BATCH // 2), rng.uniform(1.05, 40.0, N_BATCH - N_BATCH // 4 - N_BATCH // 2)])
    P = (np.asarray(pivot, D)[None, :] + d * (radius * r)[:, None]).astype(F)
    pv = np.asarray(pivot, F)
    P[:6] = [pv, pv + F([radius, 0, 0]), pv - F([0, radius, 0]), pv + F([0.75, 1.0, 0]), pv + F([3e38, 0, 0]), pv + F([1e-30, 0, 0])]
    board.set_textures([dict(flower_center=(pivot, radius))], [0, NONE])
    got, crd, undefined = _lookup3(board, 0, P)
    board.set_textures([])
    want = flower_centre_lookup(P, pivot, radius)
    err = np.abs(got.astype(D) - want.astype(D))
    print("flower centre: max abs err %.3g; red in [%.3f, %.3f]; inside %d, blending %d, beyond %d" % (
        err.max(), want[:, 0].min(), want[:, 0].max(), (want[:, 0] == F(0.31)).sum(), ((want[:, 0] > F(0.31)) & (want[:, 0] < F(0.92))).sum(),
        (want[:, 0] == F(0.92)).sum()))
    assert np.isfinite(got).all() and err.max() <= 2e-7 and undefined == 0 and (crd == 7.0).all()
    assert got[0].tolist() == [F(0.31), F(0.18), F(0.1)] and got[1].tolist() == got[2].tolist() == got[3].tolist() == [F(0.92), F(0.71), F(0.1)]
    assert ((want[:, 0] > F(0.35)) & (want[:, 0] < F(0.9))).sum() > 200 and (want[:, 0] == F(0.92)).sum() > 500 and (want[:, 0] == F(0.31)).sum() > 200


class Garden:
    """Two quads and a sphere: petal (material 0) and stem (1) on the triangles of the first quad, stone (2) and plain Phong (4) on
    those of the second, a flower centre (3) on the sphere.  The petal's pivot lies in the first quad's plane, inside the petal's
    triangle, so that the hits cover every v; the flower centre's pivot lies in front of the sphere's centre, so that the hits
    cover distances from 0.15 to 1.1 radii."""
    V = np.array([[-3, -1.5, 0.25], [0, -1.5, 0.25], [0, 1.5, 0.25], [-3, 1.5, 0.25],
                  [0.5, -1.5, -0.5], [3.5, -1.5, 0.5], [3.5, 1.5, 0.5], [0.5, 1.5, -0.5]], F)
    NRM = np.array([[0.1, 0.2, 1]] * 4 + [[-0.3, 0.1, 1]] * 4, F)
    T = np.array([[0, 0], [3, 0], [3, 3], [0, 3], [0.5, 0.25], [2.5, 0.25], [2.5, 2.25], [0.5, 2.25]], F)
    IDX = np.array([[0, 1, 2], [0, 2, 3], [4, 5, 6], [4, 6, 7]], np.uint32)
    CENTRE, RADIUS = (0.25, 0.0, 1.5), 0.75
    MATERIALS = [((1, 1, 1), (0.25, 0, 0), (0, 0, 0), 500.0, 1.5), DIFFUSE, DIFFUSE, ((1, 1, 1), (0, 0, 0), (0, 0.5, 0), 20.0, 1.5),
                 ((0.5, 0.25, 0.75), (0, 0, 0), (0, 0, 0), 1.0, 1.0)]
    PRIM_MATERIAL = [0, 1, 2, 4, 3]
    PETAL, STEM, STONE, CENTRE_TEX = dict(petal=((-1.0, -0.5, 0.25), 2.0)), dict(stem=7.5), dict(stone=3.0), dict(flower_center=((0.25, 0.0, 2.125), 0.875))

    def __init__(self, miro):
        s = miro.Scene(0)
        s.add_arrays(self.V, self.NRM, self.IDX, self.IDX)
        s.add_sphere(self.CENTRE, self.RADIUS)
        s.build(4)
        ti = np.full((5, 3), NONE, np.uint32)
        ti[:4] = self.IDX
        s.set_texcoords(self.T, ti)
        self.scene = s

    def textures(self, table, material_texture):
        self.scene.set_textures([])
        self.scene.set_materials(self.MATERIALS, self.PRIM_MATERIAL)
        if table:
            self.scene.set_textures(table, material_texture)


def garden_rays(miro, n, seed=43):
    rng = np.random.default_rng(seed)
    o = np.stack([rng.uniform(-2, 2, n), rng.uniform(-1, 1, n), rng.uniform(5, 7, n)], 1)
    tgt = np.stack([rng.uniform(-3.6, 4.1, n), rng.uniform(-1.9, 1.9, n), np.zeros(n)], 1)
    tgt[::8] = Garden.CENTRE + rng.uniform(-0.6, 0.6, (len(tgt[::8]), 3))
    d = tgt - o
    d /= np.linalg.norm(d, axis=1)[:, None]
    rays = np.zeros(n, miro.RAY_DTYPE)
    for k, name in enumerate(("ox", "oy", "oz")):
        rays[name] = o[:, k]
    for k, name in enumerate(("dx", "dy", "dz")):
        rays[name] = d[:, k]
    rays["tmin"], rays["tmax"] = 1e-4, 1e30
    return rays


@pytest.mark.gpu
def test_surface_pass_on_a_mixed_scene(miro):
    """16 384 seeded rays on the garden, mr_hit_surface with all five materials in the table.  On the UVW hits the colour is
    mr_texture_lookup3 at mr_hit_attrs' P and the normal the normalised N, bit for bit.  On every other hit colour and normal are,
    bit for bit, what mr_hit_surface writes with the UVW materials set to MR_NO_TEXTURE and the UVW textures out of the table
    (the same kernel: the UV arms are held independently by tests/test_procedural.py).  Rays that miss are untouched, and the undefined counts add up."""
    g = Garden(miro)
    s = g.scene
    g.textures([g.STEM, g.STONE], [NONE, 0, 1, NONE, NONE])
    t = Traced(miro, s, garden_rays(miro, 16384))
    old_c, old_n, old_undefined = (x.cpu().numpy() if hasattr(x, "cpu") else x for x in t.surface(s))
    g.textures([g.PETAL, g.STEM, g.STONE, g.CENTRE_TEX], [0, 1, 2, 3, NONE])
    new_c, new_n, new_undefined = (x.cpu().numpy() if hasattr(x, "cpu") else x for x in t.surface(s))
    mat = np.where(t.hit, np.asarray(g.PRIM_MATERIAL)[np.minimum(t.prim, 4)], -1)
    petal, centre = mat == 0, mat == 3
    print("garden: hits per material %s, misses %d, undefined %d (stem / stone alone %d)" % (
        [(mat == m).sum() for m in range(5)], (~t.hit).sum(), new_undefined, old_undefined))
    for m in range(5):
        assert (mat == m).sum() > 500, m
    assert (~t.hit).sum() > 500
    miss = ~t.hit
    assert (new_c[miss] == 7.0).all() and (new_n[miss] == 7.0).all()
    # the UVW hits
    rgb_p, _, undefined_p = _lookup3(s, 0, t.P[petal], coords=False)
    rgb_c, _, undefined_c = _lookup3(s, 3, t.P[centre], coords=False)
    assert same_bits(new_c[petal], rgb_p) and same_bits(new_c[centre], rgb_c) and undefined_c == 0
    assert len(np.unique(new_c[petal], axis=0)) > 100 and new_c[centre][:, 2].tolist() == [F(0.1)] * centre.sum()
    assert len(np.unique(new_c[centre][:, 0])) > 20
    for which in (petal, centre):
        assert new_n[which].tobytes() == normalised(t.N[which]).tobytes()
    # everything else
    rest = t.hit & ~petal & ~centre
    assert new_c[rest].tobytes() == old_c[rest].tobytes() and new_n[rest].tobytes() == old_n[rest].tobytes()
    assert np.abs(new_n[mat == 2] - normalised(t.N[mat == 2])).max() > 0.05            # the stone's bump is still there
    assert (new_c[mat == 4] == np.array(g.MATERIALS[4][0], F)).all()
    assert new_undefined == old_undefined + undefined_p


@pytest.mark.gpu
def test_refusals_and_routing_on_a_uvw_scene(miro):
    """mr_shade_lights, mr_shade_accumulate, mr_shade_square_lights and mr_gen_path_rays with MR_PATH_DIFFUSE: MR_ERR_STATE on a
    scene whose table holds a UVW kind, the message naming the _surface calls.  mr_texture_lookup on kind 4 and mr_texture_lookup3
    on kind 3: MR_ERR_INVALID, each naming the other.  mr_texture_bump_height on kind 4: zeros.  And a scene with only STONE / STEM
    gives the same bytes through mr_hit_surface whichever order its table has."""
    import torch
    from miro_amd import binding
    s = _stone_floor(miro, occluder=True)
    t = Traced(miro, s, _floor_rays(miro, 2051))
    n = t.n
    f32 = dict(dtype=torch.float32, device="cuda")
    rgb = torch.zeros((n, 3), **f32)
    sh_rays, sh_hits = torch.empty((n, 8), **f32), torch.empty((n, 4), **f32)
    src, cnt = torch.empty(n, dtype=torch.int32, device="cuda"), torch.zeros(1, dtype=torch.int64, device="cuda")
    s.gen_shadow_rays(t.rays, t.hits, n, FLOOR_LIGHT["position"], sh_rays, src, cnt)
    s.trace_indirect(sh_rays, cnt, n, sh_hits)
    out_rays, out_w = torch.empty((4 * n, 8), **f32), torch.empty((4 * n, 3), **f32)
    out_pix, out_ids = torch.empty(4 * n, dtype=torch.int32, device="cuda"), torch.empty(4 * n, dtype=torch.int32, device="cuda")
    cnt2 = torch.zeros(1, dtype=torch.int64, device="cuda")
    square = dict(position=(0.0, 6.0, 0.0), normal=(0.0, -1.0, 0.0), color=(1.0, 1.0, 1.0), wattage=10.0, dimensions=(1.0, 1.0))

    def path(kinds):
        return lambda: s.gen_path_rays(t.rays, t.hits, None, None, None, n, out_rays, out_w, out_pix, out_ids, cnt2, kinds=kinds)

    def calls():
        yield "mr_shade_lights", lambda: s.shade_lights(t.rays, t.hits, n, rgb)
        yield "mr_shade_accumulate", lambda: s.shade_accumulate(t.rays, t.hits, None, None, n, sh_rays, sh_hits, src, cnt,
                                                                 FLOOR_LIGHT["position"], FLOOR_LIGHT["wattage"], rgb)
        yield "mr_shade_square_lights", lambda: s.shade_square_lights([square], 4, t.rays, t.hits, n, rgb)
        yield "mr_gen_path_rays", path(binding.MR_PATH_DIFFUSE | binding.MR_PATH_MIRROR)

    for tex in UVW_TABLE:
        s.set_textures([tex], [0, NONE])
        for name, call in calls():
            with pytest.raises(miro.MiroError) as e:
                call()
            assert e.value.status == -5 and name in str(e.value) and "_surface" in str(e.value), (name, str(e.value))
        path(binding.MR_PATH_MIRROR | binding.MR_PATH_REFRACT)()
    # each lookup names the other
    s.set_textures([dict(petal=((0, 0, 0), 7.0)), dict(stem=3.0)], [0, 1])
    uv = _cuda(np.zeros((64, 3), F))
    out = torch.full((64, 3), 7.0, **f32)
    with pytest.raises(miro.MiroError) as e:
        s.texture_lookup(0, uv, 64, out)
    assert e.value.status == -1 and "mr_texture_lookup3" in str(e.value)
    with pytest.raises(miro.MiroError) as e:
        s.texture_lookup3(1, uv, 64, out)
    assert e.value.status == -1 and re.search(r"mr_texture_lookup\b(?!3)", str(e.value).split(":", 2)[2])
    assert (out == 7.0).all()
    height = torch.full((64,), 7.0, **f32)
    s.texture_bump_height(0, uv, 64, height)
    torch.cuda.synchronize()
    assert (height == 0).all()
    # STONE / STEM alone: the table's order does not matter
    s.set_textures([dict(stone=3.0), dict(stem=3.0)], [0, 1])
    a = t.surface(s)
    s.set_textures([dict(stem=3.0), dict(stone=3.0)], [1, 0])
    b = t.surface(s)
    assert a[0].cpu().numpy().tobytes() == b[0].cpu().numpy().tobytes() and a[1].cpu().numpy().tobytes() == b[1].cpu().numpy().tobytes()
    assert a[2] == b[2] and t.hit.sum() > 2000 and len(np.unique(a[0].cpu().numpy()[t.hit], axis=0)) > 1000
    s.set_textures([])
    for name, call in calls():
        call()
    torch.cuda.synchronize()
    assert float(rgb.max()) > 0


@pytest.mark.gpu
def test_flower_frame_through_render_specular(miro):
    """48 x 32, 1 spp, depth 0: FrameRenderer.render_specular on scenes.flower_scene() -- makeTestPetalScene -- equals trace ->
    mr_shade_environment -> mr_hit_surface -> mr_shade_lights_surface driven by hand, byte for byte; the petals show their
    pattern, and all four textured materials and the background are in the frame."""
    import torch
    from miro_amd import frame, scenes
    s = miro.Scene(0)
    desc = scenes.flower_setup(s)
    assert s.procedural and s.info().n_triangles == len(desc["prim_material"]) == 22593
    W, H = 48, 32
    fr = frame.FrameRenderer(s, desc, W, H, spp=1)
    fr.generate()
    per_level = fr.render_specular(depth=0, lights=desc["lights"], environment=True)
    torch.cuda.synchronize()
    got = fr.d_rgb.cpu().numpy().copy()
    n = W * H
    assert per_level[0][0] == n
    f32 = dict(dtype=torch.float32, device="cuda")
    hits, color, normal, rgb = torch.empty((n, 4), **f32), torch.full((n, 3), -1.0, **f32), torch.empty((n, 3), **f32), torch.zeros((n, 3), **f32)
    s.trace_device(fr.d_rays, n, hits)
    s.shade_environment(fr.d_rays, hits, n, rgb)
    s.hit_surface(fr.d_rays, hits, n, color, normal)
    s.shade_lights_surface(fr.d_rays, hits, color, normal, n, rgb)
    torch.cuda.synchronize()
    want = rgb.cpu().numpy()
    assert got.reshape(-1).tobytes() == want.reshape(-1).tobytes()
    prim = hits.cpu().numpy().view(miro.HIT_DTYPE).reshape(-1)["prim"]
    mat = np.where(prim == MISS, -1, np.asarray(desc["prim_material"])[np.minimum(prim, 22592)])
    c = color.cpu().numpy()
    print("flower: pixels per material %s, background %d, lit %d, petal colours %d" % (
        [(mat == m).sum() for m in range(4)], (mat == -1).sum(), (want[mat >= 0].max(axis=1) > 0).sum(), len(np.unique(c[mat == 0], axis=0))))
    assert (mat == 0).sum() > 100 and (mat == -1).sum() > 100 and (want[mat == -1] == 1).all()
    assert len(np.unique(c[mat == 0], axis=0)) > (mat == 0).sum() // 2                   # the petal pixels are not all one colour
    assert np.isfinite(want).all() and (want[mat == 0].max(axis=1) > 0).sum() > 50
