"""Procedural stone and stem textures with bump-mapped normals: the noise of csrc/mr_noise.h, StoneTexture / StemTexture and the
surface pass of csrc/mr_procedural.hip (mr_hit_surface, mr_shade_lights_surface, mr_shade_accumulate_surface,
mr_texture_bump_height, mr_noise_probe).

The oracle has no textures.  The two noise functions are pinned to tests/golden/noise_kat.npz: values recorded once, on the
CPU, from the reference's own lib/src/Perlin.cpp and lib/src/Worley.cpp (the fixture's `note` holds the compile line).  This
file restates both in numpy from the reference's lines (Perlin.h:16-51, Worley.cpp:95-173,367-436, Texture.h:20-37,192-212,
Texture.cpp:358-440, Scene.cpp:234-263), importing nothing from the product; the first test holds the restatement to the fixture
bit for bit, and the GPU tests then use it.  powf / exp of the restatement are glibc's own through ctypes: what the reference
calls.  The two integer tables are the published ones (Perlin's 2002 permutation, Worley's Poisson counts of mean 2.5)."""
import ctypes as C
import ctypes.util
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import kernel_budget  # noqa: E402

F = np.float32
D = np.float64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MISS = 0xFFFFFFFF
PLANE_BIT = 0x80000000
NONE = 0xFFFFFFFF
N_BATCH = 16 * 256 + 3                    # 16 workgroups plus a 3-lane tail
RTOL, ATOL_OF_MAX = 1e-5, 1e-7            # the project's tolerance for shaded values (tests/test_lights.py:27)
PI = F(3.1415926535897932384626433832795028841972)

PERM = np.array([
    151, 160, 137, 91, 90, 15, 131, 13, 201, 95, 96, 53, 194, 233, 7, 225, 140, 36, 103, 30, 69, 142, 8, 99, 37, 240, 21, 10, 23, 190, 6,
    148, 247, 120, 234, 75, 0, 26, 197, 62, 94, 252, 219, 203, 117, 35, 11, 32, 57, 177, 33, 88, 237, 149, 56, 87, 174, 20, 125, 136, 171,
    168, 68, 175, 74, 165, 71, 134, 139, 48, 27, 166, 77, 146, 158, 231, 83, 111, 229, 122, 60, 211, 133, 230, 220, 105, 92, 41, 55, 46,
    245, 40, 244, 102, 143, 54, 65, 25, 63, 161, 1, 216, 80, 73, 209, 76, 132, 187, 208, 89, 18, 169, 200, 196, 135, 130, 116, 188, 159,
    86, 164, 100, 109, 198, 173, 186, 3, 64, 52, 217, 226, 250, 124, 123, 5, 202, 38, 147, 118, 126, 255, 82, 85, 212, 207, 206, 59, 227,
    47, 16, 58, 17, 182, 189, 28, 42, 223, 183, 170, 213, 119, 248, 152, 2, 44, 154, 163, 70, 221, 153, 101, 155, 167, 43, 172, 9, 129,
    22, 39, 253, 19, 98, 108, 110, 79, 113, 224, 232, 178, 185, 112, 104, 218, 246, 97, 228, 251, 34, 242, 193, 238, 210, 144, 12, 191,
    179, 162, 241, 81, 51, 145, 235, 249, 14, 239, 107, 49, 192, 214, 31, 181, 199, 106, 157, 184, 84, 204, 176, 115, 121, 50, 45, 127,
    4, 150, 254, 138, 236, 205, 93, 222, 114, 67, 29, 24, 72, 243, 141, 128, 195, 78, 66, 215, 61, 156, 180] * 2, np.int64)
POISSON = np.array([
    4, 3, 1, 1, 1, 2, 4, 2, 2, 2, 5, 1, 0, 2, 1, 2, 2, 0, 4, 3, 2, 1, 2, 1, 3, 2, 2, 4, 2, 2, 5, 1, 2, 3, 2, 2, 2, 2, 2, 3, 2, 4, 2, 5, 3, 2, 2, 2, 5, 3,
    3, 5, 2, 1, 3, 3, 4, 4, 2, 3, 0, 4, 2, 2, 2, 1, 3, 2, 2, 2, 3, 3, 3, 1, 2, 0, 2, 1, 1, 2, 2, 2, 2, 5, 3, 2, 3, 2, 3, 2, 2, 1, 0, 2, 1, 1, 2, 1, 2, 2,
    1, 3, 4, 2, 2, 2, 5, 4, 2, 4, 2, 2, 5, 4, 3, 2, 2, 5, 4, 3, 3, 3, 5, 2, 2, 2, 2, 2, 3, 1, 1, 4, 2, 1, 3, 3, 4, 3, 2, 4, 3, 3, 3, 4, 5, 1, 4, 2, 4, 3,
    1, 2, 3, 5, 3, 2, 1, 3, 1, 3, 3, 3, 2, 3, 1, 5, 5, 4, 2, 2, 4, 1, 3, 4, 1, 5, 3, 3, 5, 3, 4, 3, 2, 2, 1, 1, 1, 1, 1, 2, 4, 5, 4, 5, 4, 2, 1, 5, 1, 1,
    2, 3, 3, 3, 2, 5, 2, 3, 3, 2, 0, 2, 1, 1, 4, 2, 1, 3, 2, 1, 2, 2, 3, 2, 5, 5, 3, 4, 5, 5, 2, 4, 4, 5, 3, 2, 2, 2, 1, 4, 2, 3, 3, 4, 2, 5, 4, 2, 4, 2,
    2, 2, 4, 5, 3, 2], np.int64)


# ---------------------------------------------------------------------------------------------------------------------------
# restatements (float32 numpy, the reference's order of operations; a double step is written as one)
# ---------------------------------------------------------------------------------------------------------------------------
def perlin(x, y, z):
    """PerlinNoise::noise (Perlin.h:16-51): floor, not truncation; & 255; a table of 512 entries"""
    x, y, z = (np.asarray(a, F) for a in (x, y, z))
    fx, fy, fz = np.floor(x), np.floor(y), np.floor(z)
    X, Y, Z = (f.astype(np.int64) & 255 for f in (fx, fy, fz))
    x, y, z = (x - fx).astype(F), (y - fy).astype(F), (z - fz).astype(F)

    def fade(t):
        return (t * t * t * (t * (t * F(6) - F(15)) + F(10))).astype(F)

    def lerp(t, a, b):
        return (a + t * (b - a)).astype(F)

    def grad(h, x, y, z):
        h = h & 15
        u = np.where(h < 8, x, y)
        v = np.where(h < 4, y, np.where((h == 12) | (h == 14), x, z))
        return (np.where((h & 1) == 0, u, -u) + np.where((h & 2) == 0, v, -v)).astype(F)

    u, v, w = fade(x), fade(y), fade(z)
    p = PERM
    A = p[X] + Y
    AA, AB = p[A] + Z, p[A + 1] + Z
    B = p[X + 1] + Y
    BA, BB = p[B] + Z, p[B + 1] + Z
    one = F(1)
    return lerp(w, lerp(v, lerp(u, grad(p[AA], x, y, z), grad(p[BA], x - one, y, z)),
                        lerp(u, grad(p[AB], x, y - one, z), grad(p[BB], x - one, y - one, z))),
                lerp(v, lerp(u, grad(p[AA + 1], x, y, z - one), grad(p[BA + 1], x - one, y, z - one)),
                     lerp(u, grad(p[AB + 1], x, y - one, z - one), grad(p[BB + 1], x - one, y - one, z - one))))


def generate_noise(x, y, initial_frequency, frequency_increase, amplitude_falloff, iterations):
    """generateNoise (Texture.h:20-37) with z = 0; `iterations` a number or one count per point"""
    x, y = np.asarray(x, F), np.asarray(y, F)
    it = np.broadcast_to(np.asarray(iterations), x.shape)
    amplitude, frequency = F(1), F(initial_frequency)
    value, max_val = np.zeros(x.shape, F), np.zeros(x.shape, F)
    for i in range(int(it.max())):
        on = i < it
        nz = perlin((x * frequency).astype(F), (y * frequency).astype(F), np.zeros(x.shape, F) * frequency)
        value = np.where(on, value + amplitude * nz, value).astype(F)
        max_val = np.where(on, max_val + amplitude, max_val).astype(F)
        frequency = F(frequency * F(frequency_increase))
        amplitude = F(amplitude * F(amplitude_falloff))
    return (value / max_val).astype(F)


def _lcg(s):
    return (np.uint64(1402024253) * s + np.uint64(586950981)) & np.uint64(0xFFFFFFFF)


def worley2(at):
    """WorleyNoise::noise2D(at, 3, F, delta, ID) (Worley.cpp:95-173, addSamples :367-436) for points [n, 2]: (F [n, 3] float32,
    ID [n, 3] uint32, delta [n, 3, 2] float32).  ID / delta of a slot no feature point reached stay 0."""
    at = np.asarray(at, F).reshape(-1, 2)
    n = len(at)
    Fv = np.full((n, 3), F(999999.9), F)
    ID = np.zeros((n, 3), np.uint64)
    DL = np.zeros((n, 3, 2), F)
    new = (0.398150 * at.astype(D)).astype(F)                                              # :110-111
    ia = np.floor(new).astype(np.int64)                                                     # :114-115

    def add_samples(xi, yi, mask):
        nonlocal Fv, ID, DL
        seed = ((np.int64(702395077) * xi + np.int64(915488749) * yi) & np.int64(0xFFFFFFFF)).astype(np.uint64)   # :383
        count = POISSON[(seed >> np.uint64(24)).astype(np.int64)]
        seed = _lcg(seed)
        for j in range(5):                                                                  # the table's largest count
            on = mask & (j < count)
            this_id = seed
            seed = _lcg(seed)
            fx = ((seed.astype(D) + 0.5) * (1.0 / 4294967296.0)).astype(F)                  # :397
            seed = _lcg(seed)
            fy = ((seed.astype(D) + 0.5) * (1.0 / 4294967296.0)).astype(F)
            seed = _lcg(seed)
            dx = ((xi.astype(F) + fx).astype(F) - new[:, 0]).astype(F)                      # :403-404
            dy = ((yi.astype(F) + fy).astype(F) - new[:, 1]).astype(F)
            d2 = (dx * dx + dy * dy).astype(F)
            on = on & (d2 < Fv[:, 2])                                                       # :407
            # :416-417: index = 3; while (index > 0 && d2 < F[index - 1]) index--  -- an earlier point wins a tie
            index = np.where(d2 < Fv[:, 0], 0, np.where(d2 < Fv[:, 1], 1, 2))
            dl = np.stack([dx, dy], 1)
            for slot in (2, 1):                                                             # :422-428 bump down
                move = on & (index < slot)
                Fv[move, slot], ID[move, slot], DL[move, slot] = Fv[move, slot - 1], ID[move, slot - 1], DL[move, slot - 1]
            for slot in (0, 1, 2):
                put = on & (index == slot)
                Fv[put, slot], ID[put, slot], DL[put, slot] = d2[put], this_id[put], dl[put]

    everyone = np.ones(n, bool)
    add_samples(ia[:, 0], ia[:, 1], everyone)                                               # :130
    x2 = (new[:, 0] - ia[:, 0].astype(F)).astype(F)                                         # :135-140
    y2 = (new[:, 1] - ia[:, 1].astype(F)).astype(F)
    mx2 = ((1.0 - x2.astype(D)) * (1.0 - x2.astype(D))).astype(F)
    my2 = ((1.0 - y2.astype(D)) * (1.0 - y2.astype(D))).astype(F)
    x2, y2 = (x2 * x2).astype(F), (y2 * y2).astype(F)
    for ox, oy, bound in ((-1, 0, x2), (0, -1, y2), (1, 0, mx2), (0, 1, my2),               # :146-163, each against the CURRENT F[2]
                          (-1, -1, (x2 + y2).astype(F)), (1, 1, (mx2 + my2).astype(F)),
                          (-1, 1, (x2 + my2).astype(F)), (1, -1, (mx2 + y2).astype(F))):
        add_samples(ia[:, 0] + ox, ia[:, 1] + oy, bound < Fv[:, 2])
    Fv = (np.sqrt(Fv).astype(F).astype(D) * (1.0 / 0.398150)).astype(F)                     # :169
    DL = (DL.astype(D) * (1.0 / 0.398150)).astype(F)
    return Fv, ID.astype(np.uint32), DL


_libm = C.CDLL(ctypes.util.find_library("m") or "libm.so.6")
_libm.powf.restype, _libm.powf.argtypes = C.c_float, [C.c_float, C.c_float]
_libm.exp.restype, _libm.exp.argtypes = C.c_double, [C.c_double]


def libm_powf(x, y):
    return np.array([_libm.powf(float(a), float(y)) for a in np.asarray(x, F)], F)


def libm_exp(x):
    return np.array([_libm.exp(float(a)) for a in np.asarray(x, D)], D)


def std_max(a, b):
    return np.where(a < b, b, a).astype(F)


def std_min(a, b):
    return np.where(b < a, b, a).astype(F)


def stem_lookup(uv, scale):
    """StemTexture::lookup2D (Texture.h:192-212): no transcendental; 0.3 * cells and / 2.0f promote as written"""
    uv = np.asarray(uv, F)
    u, v = (uv[:, 0] * F(scale)).astype(F), (uv[:, 1] * F(scale)).astype(F)
    f, _, _ = worley2(np.stack([u, v], 1))
    noise = generate_noise(u, v, 10, 1.5, 0.8, 10)
    cells = (f[:, 0] - f[:, 1]).astype(F)
    g = (0.5 + 0.5 * (noise + F(1)).astype(F).astype(D) / D(F(2)) - 0.3 * cells.astype(D)).astype(F)
    z = np.zeros_like(g)
    return np.stack([z, g, z], 1)


def stone_f1f0(f):
    """(1 - pow(f[1] - f[0], 0.8f)) * 1.5 (Texture.cpp:370,409) as a float"""
    return ((F(1) - libm_powf((f[:, 1] - f[:, 0]).astype(F), F(0.8))).astype(F).astype(D) * 1.5).astype(F)


def stone_height(uv, scale):
    """StoneTexture::bumpHeight2D (Texture.cpp:358-393): (height [n], f1f0 [n] as lookup2D's sign has it)"""
    uv = np.asarray(uv, F)
    u, v = (uv[:, 0] * F(scale)).astype(F), (uv[:, 1] * F(scale)).astype(F)
    f, ident, _ = worley2(np.stack([u, v], 1))
    pos = stone_f1f0(f)
    f1f0 = (pos * F(-1)).astype(F)
    height = (1.0 / (1.0 + libm_exp(-20.0 * ((f[:, 1] - f[:, 0]).astype(F).astype(D) - 0.3)))).astype(F)
    inside = f1f0.astype(D) > -1.1
    cellturb = ((generate_noise(u, v, 0.5, 2, 0.5, ident[:, 0] % 3 + 5) / F(5)).astype(F).astype(D) + 0.5).astype(F)
    turb = ((generate_noise(u, v, 1, 2, 0.5, 3) / F(10)).astype(F).astype(D) + 0.5).astype(F)
    hf = F(0.3)
    return np.where(inside, F(0.8) * cellturb + hf * height, F(1.0) * turb + hf * height).astype(F), pos


def stone_lookup(uv, scale):
    """StoneTexture::lookup2D (Texture.cpp:396-440); pow(f1f0, 2) is std::pow(float, int) of the C++03 library, a float product
    (only then does the std::min(float, float) around it compile).  Returns (rgb [n, 3], f1f0 [n])."""
    uv = np.asarray(uv, F)
    u, v = (uv[:, 0] * F(scale)).astype(F), (uv[:, 1] * F(scale)).astype(F)
    f, ident, _ = worley2(np.stack([u, v], 1))
    f1f0 = stone_f1f0(f)
    base = std_min(std_max((libm_powf(((f[:, 2] - f[:, 1]).astype(F) + f[:, 0]).astype(F), F(0.1)) - f1f0).astype(F), F(0)), F(0.5))
    id10, id5 = (ident[:, 0] % 10).astype(F), (ident[:, 0] % 5).astype(F)
    base = (base.astype(D) * ((id10 / F(20)).astype(F).astype(D) + 0.5)).astype(F)
    turb = generate_noise(u, v, 3, 2, 0.8, 5)
    base = std_max(np.zeros_like(base), base)
    base = (base.astype(D) + 0.8 * np.abs(turb).astype(D)).astype(F)
    edges = std_min((f1f0 * f1f0 - F(1)).astype(F), F(0.75))
    grey = (edges.astype(D) + 0.25 * np.abs(turb).astype(D)).astype(F)
    rgb = np.stack([(base + id10 / F(10)).astype(F), (base + (id10 / F(10)).astype(F) * F(0.5)).astype(F),
                    (base + (id5 / F(5)).astype(F) * F(0.25)).astype(F)], 1)
    edge = f1f0.astype(D) > 1.1
    return np.where(edge[:, None], grey[:, None], rgb).astype(F), f1f0


def dot3(a, b):
    return ((a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]).astype(F) + a[:, 2] * b[:, 2]).astype(F)


def cross3(a, b):
    return np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2], a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], 1).astype(F)


def normalised(N):
    """Vector3::normalize (Scene.cpp:262): *= 1 / length"""
    return (N * (F(1) / np.sqrt(dot3(N, N)))[:, None]).astype(F)


def bumped_normal(N, u1, u2, v1, v2):
    """Scene.cpp:249-262 on the normal N as intersect() left it and the four heights"""
    delta = F(0.0001)
    dx, dy = ((u2 - u1) / (F(2) * delta)).astype(F), ((v2 - v1) / (F(2) * delta)).astype(F)
    m = np.where(N[:, 1] > N[:, 0], 1, 0)
    m = np.where(N[:, 2] > N[np.arange(len(N)), m], 2, m)
    zero = np.zeros(len(N), F)
    r = np.stack([np.where(m == 2, -N[:, 2], zero), np.where(m == 0, -N[:, 0], zero), np.where(m == 1, -N[:, 1], zero)], 1).astype(F)
    t1 = cross3(N, r)
    c1 = cross3(N, t1)
    c2 = cross3(N, c1)
    out = (N + ((c1 * dx[:, None]).astype(F) - (c2 * dy[:, None]).astype(F)).astype(F)).astype(F)
    return normalised(out), m


def ulp_distance(a, b):
    """distance in units of the last place between two float32 arrays of one sign pattern (ordered-integer difference)"""
    def key(x):
        i = np.asarray(x, F).view(np.int32).astype(np.int64)
        return np.where(i < 0, np.int64(-0x80000000) - i, i)
    return np.abs(key(a) - key(b))


# ---------------------------------------------------------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def kat(golden_dir):
    z = np.load(os.path.join(golden_dir, "noise_kat.npz"))
    return {k: z[k] for k in z.files}


def test_restatement_equals_the_recorded_reference_values(kat):
    """Both noises, restated above, against values recorded from the reference's own Perlin.cpp / Worley.cpp: bit for bit, ids
    and deltas included; and the fixture holds the cases that make it worth having."""
    assert "lib/src/Perlin.cpp" in str(kat["note"]) and "-ffp-contract=off" in str(kat["note"])
    p = kat["perlin_xyz"]
    assert len(p) >= 2000 and (p[:, 2] != 0).sum() > 1000 and (p < 0).any() and (p == np.floor(p)).all(axis=1).any()
    assert ((p[:, 0] >= 254.5) & (p[:, 0] <= 257.5)).sum() >= 100 and (p[:, 0] == F(-0.5)).any()
    assert perlin(p[:, 0], p[:, 1], p[:, 2]).tobytes() == kat["perlin"].tobytes()
    at = kat["worley_at"]
    cell = at.astype(D) * 0.398150
    assert len(at) >= 2000 and (at < 0).any() and (at == 0).all(axis=1).any()
    assert (np.abs(cell - np.round(cell)).min(axis=1) < 1e-6).sum() >= 100             # within 1e-6 of a cell border
    f, ident, delta = worley2(at)
    assert f.tobytes() == kat["worley_F"].tobytes()
    assert np.array_equal(ident, kat["worley_ID"])
    assert delta.tobytes() == kat["worley_delta"].tobytes()
    # the anchor point
    f, ident, _ = worley2(np.array([[0.3, -1.7]], F))
    assert [float(x).hex() for x in f[0]] == ["0x1.e2a5500000000p-1", "0x1.52b6a80000000p+0", "0x1.5c55ca0000000p+0"]
    assert ident[0].tolist() == [953543893, 483222413, 1859188819]
    assert float(perlin(F(0.3), F(-1.7), F(0))).hex() == "0x1.39018c0000000p-1"


def _host_scene(miro):
    s = miro.Scene()
    s.add_triangle([0, 0, 0, 1, 0, 0, 0, 1, 0], [0, 0, 1] * 3)
    s.add_triangle([0, 0, 1, 1, 0, 1, 0, 1, 1], [0, 0, 1] * 3)
    s.build(4, host_only=True)
    return s


DIFFUSE = ((1, 1, 1), (0, 0, 0), (0, 0, 0), 20.0, 1.0)
SHINY = ((1, 1, 1), (0.25, 0, 0), (0, 0, 0), 20.0, 1.0)
GLASSY = ((1, 1, 1), (0, 0, 0), (0, 0.5, 0), 20.0, 1.5)


def test_set_textures_accepts_stone_and_stem_on_a_host_only_scene(miro):
    from miro_amd import binding
    assert (binding.MR_TEX_STONE, binding.MR_TEX_STEM) == (2, 3)
    s = _host_scene(miro)
    s.set_materials([DIFFUSE, SHINY], [0, 1])
    s.set_textures([dict(stone=3.0), dict(stem=1.0)], [0, 1])          # a STEM may sit on a specular material
    assert s.procedural
    with pytest.raises(miro.MiroError) as e:                             # the table is there: it names materials by index
        s.set_materials([DIFFUSE, SHINY], [0, 1])
    assert e.value.status == -5
    s.set_textures([])
    assert not s.procedural
    s.set_materials([DIFFUSE, SHINY], [0, 1])


def test_set_textures_refuses_bad_procedural_textures_and_keeps_the_earlier_table(miro):
    from miro_amd import binding
    s = _host_scene(miro)
    L = miro.lib()
    mats = [DIFFUSE, SHINY, GLASSY]
    s.set_materials(mats, [0, 1])
    s.set_textures([dict(color1=(1, 1, 1), color2=(0, 0, 0), scale=2.0)], [0, NONE, NONE])

    def table_still_there():
        with pytest.raises(miro.MiroError) as e:
            s.set_materials(mats, [0, 1])
        return e.value.status == -5

    def desc(kind, scale, reserved=0):
        d = binding.TextureDesc()
        d.kind, d.scale = kind, scale
        d.reserved[1] = reserved
        return d

    ok = np.array([0, NONE, NONE], np.uint32)
    for kind in (binding.MR_TEX_STONE, binding.MR_TEX_STEM):
        for bad in (desc(kind, np.nan), desc(kind, np.inf), desc(kind, -np.inf), desc(kind, 1.0, reserved=1)):
            assert L.mr_scene_set_textures(s.h, (binding.TextureDesc * 1)(bad), 1, binding._u32p(ok)) == -1, L.mr_last_error()
            assert table_still_there()
    stone = (binding.TextureDesc * 1)(desc(binding.MR_TEX_STONE, 3.0))
    for mt in ([NONE, 0, NONE], [NONE, NONE, 0], [0, 0, NONE]):         # ks != 0, kt != 0
        assert L.mr_scene_set_textures(s.h, stone, 1, binding._u32p(np.array(mt, np.uint32))) == -1
        assert b"STONE" in L.mr_last_error() and table_still_there()
    stem = (binding.TextureDesc * 1)(desc(binding.MR_TEX_STEM, 3.0))
    assert L.mr_scene_set_textures(s.h, stem, 1, binding._u32p(np.array([0, 0, 0], np.uint32))) == 0
    assert L.mr_scene_set_textures(s.h, stone, 1, binding._u32p(ok)) == 0


def test_procedural_kernels_stay_inside_the_verified_envelope():
    """Every kernel of mr_procedural.hip (remarks in build/mr_procedural.remarks.txt), 18 of them: no dynamic stack; no more spilled
    VGPRs, no more scratch per lane and no fewer waves per SIMD than BOTH its own record (tests/golden/kernel_budget_procedural.json,
    written by tools/kernel_budget.py --write-unit mr_procedural from the build whose GPU run of this file, of
    tests/test_solid_textures.py and of tests/test_photon_walk_surface.py was green) AND the worst value among the kernels of
    tests/golden/kernel_budget.json.  The one surface pass (hit_surface_kernel, every scene's) and the inspection kernels, the
    UVW one included, have no traversal: no scratch at all."""
    cur = kernel_budget.unit_kernels("mr_procedural")
    count = lambda word: sum(word in k for k in cur)                                         # noqa: E731
    assert len(cur) == 18 and count("shade_lights_surf_kernel") == 12
    for word in ("hit_surface_kernel", "shade_accumulate_surf_kernel", "texture_lookup_proc_kernel", "texture_lookup3_kernel",
                 "bump_height_kernel", "noise_probe_kernel"):
        assert count(word) == 1, word
        name = [k for k in cur if word in k][0]
        assert cur[name]["scratch_bytes_per_lane"] == 0 and cur[name]["vgprs_spilled"] == 0, (name, cur[name])
    kernel_budget.assert_inside_envelope(cur, "kernel_budget_procedural.json", also_main=True)


def test_the_procedural_entries_are_exported_and_declared(miro):
    import re
    src = open(os.path.join(ROOT, "include", "miro_hip.h")).read()
    L = miro.lib()
    for name in ("mr_hit_surface", "mr_shade_lights_surface", "mr_shade_accumulate_surface", "mr_texture_bump_height", "mr_noise_probe"):
        assert hasattr(L, name) and name in miro.EXPORTED_SYMBOLS and re.search(r"\b%s\s*\(" % name, src), name
    assert re.search(r"MR_TEX_STONE = 2, MR_TEX_STEM = 3", src) and re.search(r"MR_NOISE_PERLIN = 0, MR_NOISE_WORLEY2 = 1", src)
    dummy = C.c_void_p(16)
    assert L.mr_noise_probe(2, dummy, 4, dummy, None) == -1 and L.mr_noise_probe(0, None, 4, dummy, None) == -1
    s = _host_scene(miro)                                                # no device: MR_ERR_STATE, never a CPU path
    assert L.mr_hit_surface(s.h, dummy, dummy, 4, dummy, dummy, None, None) == -5
    assert L.mr_texture_bump_height(s.h, 0, dummy, 4, dummy, None) == -5


# ---------------------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------------------
def _cuda(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _pad(a, n=N_BATCH):
    """the first n rows of `a` repeated as often as it takes"""
    reps = -(-n // len(a))
    return np.concatenate([a] * reps)[:n]


@pytest.mark.gpu
def test_noise_probe_equals_the_recorded_reference_values(miro, kat):
    """mr_noise_probe for both noises against the fixture: array_equal, ids included.  4 099 points: the fixture's, repeated."""
    import torch
    from miro_amd import binding
    p = _pad(kat["perlin_xyz"])
    out = torch.full((N_BATCH,), 7.0, dtype=torch.float32, device="cuda")
    binding.noise_probe(binding.MR_NOISE_PERLIN, _cuda(p), N_BATCH, out)
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy().view(np.uint32), _pad(kat["perlin"]).view(np.uint32))
    at = _pad(kat["worley_at"])
    out = torch.full((N_BATCH, 6), 7.0, dtype=torch.float32, device="cuda")
    binding.noise_probe(binding.MR_NOISE_WORLEY2, _cuda(at), N_BATCH, out)
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert np.array_equal(got[:, :3].view(np.uint32), _pad(kat["worley_F"]).view(np.uint32))
    assert np.array_equal(got[:, 3:].copy().view(np.uint32), _pad(kat["worley_ID"]))
    # what the reference leaves undefined is defined: noise 0
    bad = np.array([[np.nan, 0, 0], [0, 2.0 ** 30, 0], [0, 0, -np.inf], [1.5, 2.5, 3.5]], F)
    out = torch.full((4,), 7.0, dtype=torch.float32, device="cuda")
    binding.noise_probe(binding.MR_NOISE_PERLIN, _cuda(bad), 4, out)
    torch.cuda.synchronize()
    assert (out.cpu().numpy()[:3] == 0).all() and out.cpu().numpy()[3] == perlin(F(1.5), F(2.5), F(3.5))


class Yard:
    """A floor plane (material 0), a sphere (1), a mesh with texture coordinates facing +x, +y and +z (2), a triangle without
    texture coordinates (3), a small opaque sphere that shades the floor (4), a checkered triangle (5)."""
    TEX_V = np.array([[3, 0.2, -1], [3, 2.2, 0], [3, 0.2, 1],            # cross(B - A, C - A) = (+4, 0, 0)
                      [-4, 0.5, -1], [-4, 0.5, 1], [-2, 0.5, 0],         # cross = (0, +4, 0)
                      [-1, 0.2, -3], [1, 0.2, -3], [0, 2.2, -3]], F)     # cross = (0, 0, +4)
    TEX_N = np.array([[1, 0.1, 0.2]] * 3 + [[0.2, 1, 0.1]] * 3 + [[0.1, 0.2, 1]] * 3, F)      # largest component x, y, z
    TEX_T = np.array([[0, 0], [1, 0], [0.5, 1], [0.1, 0.2], [0.9, 0.1], [0.4, 0.8], [2, 2], [3, 2], [2.5, 3.5]], F)
    PLAIN_V = np.array([[-2, 0.3, -2.5], [-0.5, 0.3, -2.5], [-1.2, 1.8, -2.0]], F)
    CHECK_V = np.array([[1.5, 0.3, 2.5], [3.0, 0.3, 2.5], [2.2, 1.8, 2.0]], F)
    CENTRE, RADIUS = (0.0, 1.0, 0.0), 1.0
    SHADE = ((1.2, 2.6, 0.6), 0.5)
    LIGHTS = [dict(position=(2.0, 6.0, 1.0), color=(1.0, 0.9, 0.8), wattage=400.0),
              dict(position=(-1.0, 7.0, -0.5), normal=(0.0, -2.0, 0.0), color=(0.8, 0.9, 1.0), wattage=3.0, radius=6.0)]
    MATERIALS = [((0.7, 0.6, 0.5), (0, 0, 0), (0, 0, 0), 20.0, 1.0)] * 4 + [((0.5, 0.25, 0.75), (0, 0, 0), (0, 0, 0), 1.0, 1.0),
                                                                         ((0.3, 0.3, 0.3), (0.25, 0, 0.125), (0, 0, 0), 20.0, 1.0)]
    CHECKER = dict(color1=(1.0, 0.5, 0.25), color2=(0.125, 0.25, 0.5), scale=10.0)

    def __init__(self, miro):
        s = miro.Scene(0)
        self.sphere = s.add_sphere(self.CENTRE, self.RADIUS)
        n3 = len(self.TEX_V) // 3
        idx = np.arange(len(self.TEX_V)).reshape(-1, 3)
        s.add_arrays(self.TEX_V, self.TEX_N, idx, idx)                   # objects 1 ... 3
        self.plain = 1 + n3
        up = np.tile(np.array([[0, 0.5, 2]], F), (3, 1))
        s.add_arrays(self.PLAIN_V, up, [[0, 1, 2]], [[0, 1, 2]])
        self.shade = s.add_sphere(*self.SHADE)
        self.check = self.shade + 1
        s.add_arrays(self.CHECK_V, up, [[0, 1, 2]], [[0, 1, 2]])
        s.add_plane((0, 2, 0), (0, 0, 0), 0)                             # a normal that is not of unit length
        self.n_obj = self.check + 1
        self.prim_material = np.array([1] + [2] * n3 + [3, 4, 5], np.uint32)
        ti = np.full((self.n_obj, 3), NONE, np.uint32)
        ti[1:1 + n3] = idx
        ti[self.check] = [0, 1, 2]
        s.build(4)
        s.set_texcoords(self.TEX_T, ti)
        s.set_lights(self.LIGHTS)
        self.scene, self.n_tex_tris = s, n3
        self.untextured()

    def untextured(self):
        self.scene.set_textures([])
        self.scene.set_materials(self.MATERIALS, self.prim_material)

    def stone(self, scale=3.0):
        """stone on the floor, the sphere, both meshes (textures 0); plain Phong on the small sphere; checker 1 on the last triangle"""
        self.untextured()
        self.scene.set_textures([dict(stone=scale), self.CHECKER], [0, 0, 0, 0, NONE, 1])

    def material_of(self, prim):
        return np.where(prim == MISS, 0, np.where((prim & PLANE_BIT) != 0, 0, self.prim_material[np.minimum(prim, self.n_obj - 1)]))


def yard_rays(miro, n, seed=5):
    rng = np.random.default_rng(seed)
    o = np.stack([rng.uniform(-5, 5, n), rng.uniform(2.5, 7, n), rng.uniform(-5, 5, n)], axis=1)
    tgt = np.stack([rng.uniform(-5, 5, n), rng.uniform(-0.5, 2.5, n), rng.uniform(-5, 5, n)], axis=1)
    tgt[::8, 1] = 12.0
    tris = np.concatenate([Yard.TEX_V, Yard.PLAIN_V, Yard.CHECK_V]).astype(D).reshape(-1, 3, 3)
    for c, k in enumerate(range(1, n, 4)):
        tgt[k] = rng.dirichlet((1, 1, 1)) @ tris[c % len(tris)]
    for k in range(2, n, 8):
        tgt[k] = np.asarray(Yard.CENTRE) + rng.uniform(-0.6, 0.6, 3)
    d = tgt - o
    d /= np.linalg.norm(d, axis=1)[:, None]
    rays = np.zeros(n, miro.RAY_DTYPE)
    for k, name in enumerate(("ox", "oy", "oz")):
        rays[name] = o[:, k]
    for k, name in enumerate(("dx", "dy", "dz")):
        rays[name] = d[:, k]
    rays["tmin"], rays["tmax"] = 1e-4, 1e30
    return rays


class Traced:
    """A batch of rays traced against a scene, with what the tests read back of it"""

    def __init__(self, miro, scene, rays):
        import torch
        self.n = n = len(rays)
        self.rays_np = rays
        self.rays = _cuda(rays.view(F).reshape(n, 8).copy())
        self.hits = torch.empty((n, 4), dtype=torch.float32, device="cuda")
        scene.trace_device(self.rays, n, self.hits)
        P = torch.empty((n, 3), dtype=torch.float32, device="cuda")
        N = torch.empty((n, 3), dtype=torch.float32, device="cuda")
        uv = torch.empty((n, 2), dtype=torch.float32, device="cuda")
        scene.hit_attrs(self.hits, n, P, N, d_rays=self.rays)
        scene.hit_uv(self.rays, self.hits, n, uv)
        torch.cuda.synchronize()
        self.P, self.N, self.uv, self.d_uv = P.cpu().numpy(), N.cpu().numpy(), uv.cpu().numpy(), uv
        self.prim = self.hits.cpu().numpy().view(miro.HIT_DTYPE).reshape(-1)["prim"]
        self.hit = self.prim != MISS

    def surface(self, scene, fill=7.0):
        import torch
        color = torch.full((self.n, 3), fill, dtype=torch.float32, device="cuda")
        normal = torch.full((self.n, 3), fill, dtype=torch.float32, device="cuda")
        counts = torch.zeros(1, dtype=torch.int64, device="cuda")
        scene.hit_surface(self.rays, self.hits, self.n, color, normal, d_counts=counts)
        torch.cuda.synchronize()
        return color, normal, int(counts.item())


@pytest.fixture(scope="module")
def yard(miro):
    return Yard(miro)


@pytest.fixture(scope="module")
def traced(miro, yard):
    return Traced(miro, yard.scene, yard_rays(miro, N_BATCH))


def _lookup(scene, texture, uv):
    import torch
    n = len(uv)
    rgb = torch.full((n, 3), 7.0, dtype=torch.float32, device="cuda")
    counts = torch.zeros(1, dtype=torch.int64, device="cuda")
    scene.texture_lookup(texture, uv if isinstance(uv, torch.Tensor) else _cuda(np.asarray(uv, F)), n, rgb, d_counts=counts)
    torch.cuda.synchronize()
    return rgb.cpu().numpy(), int(counts.item())


def _heights(scene, texture, uv):
    import torch
    n = len(uv)
    h = torch.full((n,), 7.0, dtype=torch.float32, device="cuda")
    scene.texture_bump_height(texture, _cuda(np.asarray(uv, F)), n, h)
    torch.cuda.synchronize()
    return h.cpu().numpy()


@pytest.mark.gpu
def test_stem_lookup_is_bit_equal(miro, yard):
    """StemTexture::lookup2D has no transcendental: mr_texture_lookup equals the restatement bit for bit, at two scales, negative
    coordinates included; its bump height is 0; an undefined coordinate is green 0.5 + ... of noise 0 and counted."""
    rng = np.random.default_rng(11)
    uv = rng.uniform(-3, 3, (N_BATCH, 2)).astype(F)
    uv[:4] = [[0, 0], [0.3, -1.7], [-0.5, -0.5], [1, 1]]
    for scale in (1.0, 7.5):
        yard.untextured()
        yard.scene.set_textures([dict(stem=scale)], [0, NONE, NONE, NONE, NONE, NONE])
        got, undefined = _lookup(yard.scene, 0, uv)
        want = stem_lookup(uv, scale)
        assert got.tobytes() == want.tobytes() and undefined == 0
        assert (got[:, 0] == 0).all() and (got[:, 2] == 0).all() and got[:, 1].std() > 0.01
        assert (_heights(yard.scene, 0, uv[:300]) == 0).all()
    bad = np.array([[np.nan, 0], [3e38, 3e38], [0.5, 0.5]], F)
    got, undefined = _lookup(yard.scene, 0, bad)
    assert undefined == 2 and np.isfinite(got).all()
    yard.untextured()


STONE_ULP_BOUND = 1


@pytest.mark.gpu
@pytest.mark.parametrize("scale", [3.0, 20.0])
def test_stone_colour_and_height_against_the_restatement(miro, yard, scale):
    """StoneTexture::lookup2D and ::bumpHeight2D on a 96 x 96 grid over [-2, 2]^2 against the restatement, whose powf / exp are
    glibc's (what the reference calls) where the device evaluates miro_math.h's double series rounded once.  Both functions
    branch on f1f0 against +-1.1: points with |f1f0 - 1.1| < 1e-3 in the restatement are left out, at most 1 % of the grid.
    Heights: within STONE_ULP_BOUND ulp -- the measured maximum on this grid (MI355X, both scales) rounded up to the next power
    of two; measured: see DESIGN section 4.  Colours: within 1e-6 absolute.  Where that comes from: every channel is a sum of
    terms of magnitude <= 1.5; the two powf results entering it are within 1 ulp of glibc's (the height bound), 1.8e-7 on
    f1f0 <= 1.5 after its factor 1.5, twice that on edges = f1f0^2 - 1 (5.4e-7), and one more rounding each on the sums."""
    g = np.linspace(-2, 2, 96).astype(F)
    uv = np.stack(np.meshgrid(g, g), -1).reshape(-1, 2).astype(F)
    yard.untextured()
    yard.scene.set_textures([dict(stone=scale)], [0, NONE, NONE, NONE, NONE, NONE])
    got_h = _heights(yard.scene, 0, uv)
    got_c, undefined = _lookup(yard.scene, 0, uv)
    yard.untextured()
    want_h, f1f0 = stone_height(uv, scale)
    want_c, f1f0_c = stone_lookup(uv, scale)
    assert np.array_equal(f1f0, f1f0_c) and undefined == 0
    keep = np.abs(f1f0.astype(D) - 1.1) >= 1e-3
    ulp = ulp_distance(got_h[keep], want_h[keep])
    err_c = np.abs(got_c[keep].astype(D) - want_c[keep].astype(D))
    print("stone scale %g: left out %d of %d; heights max ulp %d (exact %d of %d), range [%.3f, %.3f]; colour max abs err %.3g; "
          "edge points %d" % (scale, (~keep).sum(), len(uv), ulp.max(), (ulp == 0).sum(), keep.sum(), want_h.min(), want_h.max(),
                              err_c.max(), (f1f0 > 1.1).sum()))
    assert (~keep).sum() <= 0.01 * len(uv)
    assert (f1f0 > 1.1).sum() > 50 and (f1f0 <= 1.1).sum() > 50                       # both branches of both functions
    assert ulp.max() <= STONE_ULP_BOUND
    assert err_c.max() <= 1e-6
    assert want_c.std() > 0.05 and want_h.std() > 0.01


@pytest.mark.gpu
def test_bump_mapped_normals_from_the_devices_own_heights(miro, yard, traced):
    """The bump arithmetic apart from the transcendentals: (u, v) from mr_hit_uv, u -+ delta and v -+ delta formed in float32,
    the four heights from mr_texture_bump_height itself, Scene.cpp:249-262 restated in float32 -- mr_hit_surface's normals agree
    within RTOL / ATOL_OF_MAX.  (Against restated heights a last-bit difference would be multiplied by 1 / delta = 1e4 in dx.)
    All three arms of randomVec are taken.  The triangle without texture coordinates has uv = (0, 0) at every hit: its four
    samples lie at (-+delta, 0) and (0, -+delta), the same four for every hit, so dx and dy are one pair of constants -- not
    zero: the height is not flat around the origin -- and its normal is bumped like the others.  Plain and checker materials:
    colour = m_diffuse / mr_texture_lookup bit for bit, N only normalised."""
    scale = 3.0
    yard.stone(scale)
    s, t = yard.scene, traced
    color, normal, undefined = t.surface(s)
    color, normal = color.cpu().numpy(), normal.cpu().numpy()
    mat = yard.material_of(t.prim)
    miss = ~t.hit
    assert undefined == 0 and miss.sum() > 100
    assert (color[miss] == 7.0).all() and (normal[miss] == 7.0).all()               # a miss writes nothing
    stone = t.hit & (mat <= 3)
    delta = F(0.0001)
    u, v = t.uv[stone, 0], t.uv[stone, 1]
    h = [_heights(s, 0, np.stack(p, 1)) for p in (((u - delta).astype(F), v), ((u + delta).astype(F), v),
                                                  (u, (v - delta).astype(F)), (u, (v + delta).astype(F)))]
    want, arm = bumped_normal(t.N[stone], *h)
    err = np.abs(normal[stone] - want)
    plainly = normalised(t.N[stone])
    moved = np.abs(want - plainly).max(axis=1)
    print("bump: stone hits %d (plane %d sphere %d mesh %d bare %d), arms %s, max abs err %.3g, normals moved by up to %.3g" % (
        stone.sum(), (mat[stone] == 0).sum(), (mat[stone] == 1).sum(), (mat[stone] == 2).sum(), (mat[stone] == 3).sum(),
        np.bincount(arm, minlength=3).tolist(), err.max(), moved.max()))
    for m_id in (0, 1, 2, 3):
        assert (mat[stone] == m_id).sum() > 30, m_id
    assert (np.bincount(arm, minlength=3) > 30).all()                                # x, y and z
    assert (err <= RTOL * np.abs(want) + ATOL_OF_MAX * np.abs(want).max()).all()
    assert np.abs(dot3(normal[stone], normal[stone]) - 1).max() < 1e-6
    assert moved.max() > 0.05                                                        # the bump shows
    bare = mat[stone] == 3                                                           # no texture coordinates: uv = (0, 0)
    assert (t.uv[stone][bare] == 0).all()
    for k in range(4):                                                               # one set of four heights for all its hits
        assert len(np.unique(h[k][bare])) == 1
    assert normal[stone][bare].tobytes() == want[bare].tobytes()                     # (N itself is interpolated per hit)
    assert np.abs(normal[stone][bare] - plainly[bare]).max() > 0.05
    # the stone colour is the lookup's
    rgb, _ = _lookup(s, 0, t.d_uv)
    assert color[stone].tobytes() == rgb[stone].tobytes()
    # plain Phong and checker
    plain = t.hit & (mat == 4)
    check = t.hit & (mat == 5)
    assert plain.sum() > 20 and check.sum() > 20
    assert (color[plain] == np.array(Yard.MATERIALS[4][0], F)).all()
    rgb, _ = _lookup(s, 1, t.d_uv)
    assert color[check].tobytes() == rgb[check].tobytes() and len(np.unique(color[check], axis=0)) == 2
    for which in (plain, check):
        assert normal[which].tobytes() == normalised(t.N[which]).tobytes()
    yard.untextured()


class Plot:
    """Two quads and a sphere: a checker (material 0) and an 8 x 8 seeded image (1) on the triangles of the first quad, stem (2) and
    stone (3) on those of the second, plain Phong (4) on the sphere."""
    V = np.array([[-3, -1.5, 0.25], [0, -1.5, 0.25], [0, 1.5, 0.25], [-3, 1.5, 0.25],
                  [0.5, -1.5, -0.5], [3.5, -1.5, 0.5], [3.5, 1.5, 0.5], [0.5, 1.5, -0.5]], F)
    NRM = np.array([[0.1, 0.2, 1]] * 4 + [[-0.3, 0.1, 1]] * 4, F)
    T = np.array([[0, 0], [3, 0], [3, 3], [0, 3], [0.5, 0.25], [2.5, 0.25], [2.5, 2.25], [0.5, 2.25]], F)
    IDX = np.array([[0, 1, 2], [0, 2, 3], [4, 5, 6], [4, 6, 7]], np.uint32)
    CENTRE, RADIUS = (0.25, 0.0, 1.5), 0.75
    MATERIALS = [((1, 1, 1), (0.25, 0, 0), (0, 0, 0), 500.0, 1.5), DIFFUSE, DIFFUSE, DIFFUSE, ((0.5, 0.25, 0.75), (0, 0, 0), (0, 0, 0), 1.0, 1.0)]
    PRIM_MATERIAL = [0, 1, 2, 3, 4]
    TABLE = [dict(color1=(1.0, 0.5, 0.25), color2=(0.125, 0.25, 0.5), scale=4.0),
             dict(pixels=np.random.default_rng(47).random((8, 8, 3)).astype(F)), dict(stem=7.5), dict(stone=3.0)]
    MATERIAL_TEXTURE = [0, 1, 2, 3, NONE]

    def __init__(self, miro):
        s = miro.Scene(0)
        s.add_arrays(self.V, self.NRM, self.IDX, self.IDX)
        s.add_sphere(self.CENTRE, self.RADIUS)
        s.build(4)
        ti = np.full((5, 3), NONE, np.uint32)
        ti[:4] = self.IDX
        s.set_texcoords(self.T, ti)
        s.set_materials(self.MATERIALS, self.PRIM_MATERIAL)
        s.set_textures(self.TABLE, self.MATERIAL_TEXTURE)
        self.scene = s


def plot_rays(miro, n, seed=43):
    rng = np.random.default_rng(seed)
    o = np.stack([rng.uniform(-2, 2, n), rng.uniform(-1, 1, n), rng.uniform(5, 7, n)], 1)
    tgt = np.stack([rng.uniform(-3.6, 4.1, n), rng.uniform(-1.9, 1.9, n), np.zeros(n)], 1)
    tgt[::8] = Plot.CENTRE + rng.uniform(-0.6, 0.6, (len(tgt[::8]), 3))
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
def test_surface_pass_colours_are_the_2d_lookups_at_the_hits_own_uv(miro):
    """The UV arms of the one surface kernel, held by something that is not the surface pass: 4 099 seeded rays (16 workgroups and
    a 3-lane tail) on a scene whose table holds a CHECKER, an IMAGE, a STEM and a STONE next to a plain material.  The colour of
    every textured hit is mr_texture_lookup of its texture at mr_hit_uv's (u, v), bit for bit; a plain hit's is the material's
    kd; the normal of every hit that is not on the stone is the normalised mr_hit_attrs normal, byte for byte (the stone's bumped
    normals are test_bump_mapped_normals_from_the_devices_own_heights'); rays that miss keep the fill value; the undefined count
    is the sum of the lookups' counts."""
    p = Plot(miro)
    s = p.scene
    t = Traced(miro, s, plot_rays(miro, N_BATCH))
    color, normal, undefined = t.surface(s)
    color, normal = color.cpu().numpy(), normal.cpu().numpy()
    mat = np.where(t.hit, np.asarray(p.PRIM_MATERIAL)[np.minimum(t.prim, 4)], -1)
    print("plot: hits per material %s, misses %d, undefined %d" % ([(mat == m).sum() for m in range(5)], (mat == -1).sum(), undefined))
    for m in range(-1, 5):
        assert (mat == m).sum() >= 100, m
    miss = mat == -1
    assert (color[miss] == 7.0).all() and (normal[miss] == 7.0).all()
    looked_up_undefined = 0
    for m, tex in enumerate(p.MATERIAL_TEXTURE[:4]):
        which = mat == m
        rgb, count = _lookup(s, tex, t.uv[which])
        assert color[which].tobytes() == rgb.tobytes(), m
        assert len(np.unique(rgb, axis=0)) > (1 if m == 0 else 20), m                    # a checker has two colours
        looked_up_undefined += count
    assert len(np.unique(color[mat == 0], axis=0)) == 2
    assert (color[mat == 4] == np.array(p.MATERIALS[4][0], F)).all()
    flat = t.hit & (mat != 3)
    assert normal[flat].tobytes() == normalised(t.N[flat]).tobytes()
    assert np.abs(normal[mat == 3] - normalised(t.N[mat == 3])).max() > 0.05            # the stone's bump is there
    assert undefined == looked_up_undefined


def _chain(scene, t, light, surface=None):
    import torch
    n = t.n
    sh_rays = torch.empty((n, 8), dtype=torch.float32, device="cuda")
    sh_hits = torch.empty((n, 4), dtype=torch.float32, device="cuda")
    src = torch.empty(n, dtype=torch.int32, device="cuda")
    cnt = torch.zeros(1, dtype=torch.int64, device="cuda")
    rgb = torch.zeros((n, 3), dtype=torch.float32, device="cuda")
    scene.gen_shadow_rays(t.rays, t.hits, n, light["position"], sh_rays, src, cnt)
    scene.trace_indirect(sh_rays, cnt, n, sh_hits)
    if surface is None:
        scene.shade_accumulate(t.rays, t.hits, None, None, n, sh_rays, sh_hits, src, cnt, light["position"], light["wattage"], rgb,
                               color=light["color"])
    else:
        scene.shade_accumulate_surface(t.rays, t.hits, surface[0], surface[1], None, None, n, sh_rays, sh_hits, src, cnt,
                                       light["position"], light["wattage"], rgb, color=light["color"])
    torch.cuda.synchronize()
    return rgb.cpu().numpy()


@pytest.mark.gpu
def test_surface_shading_reproduces_the_plain_calls_on_an_untextured_scene(miro, yard, traced):
    """No texture: mr_hit_surface gives d_color = m_diffuse and d_normal = the normalised normal, and with them
    mr_shade_lights_surface / mr_shade_accumulate_surface reproduce mr_shade_lights (a point and a disc light) /
    mr_shade_accumulate within RTOL / ATOL_OF_MAX.  The small opaque sphere shades part of the floor: the shadow traversal of
    the _surface kernel decides those rays."""
    import torch
    yard.untextured()
    s, t = yard.scene, traced
    color, normal, _ = t.surface(s, fill=0.0)
    mat = yard.material_of(t.prim)
    want_c = np.array([m[0] for m in Yard.MATERIALS], F)[mat]
    assert (color.cpu().numpy()[t.hit] == want_c[t.hit]).all()
    out = {}
    for name in ("plain", "surface"):
        ray_rgb = torch.zeros((t.n, 3), dtype=torch.float32, device="cuda")
        rgb = torch.zeros((t.n, 3), dtype=torch.float32, device="cuda")
        cnt = torch.zeros(1, dtype=torch.int64, device="cuda")
        if name == "plain":
            s.shade_lights(t.rays, t.hits, t.n, rgb, d_ray_rgb=ray_rgb, d_counts=cnt)
        else:
            s.shade_lights_surface(t.rays, t.hits, color, normal, t.n, rgb, d_ray_rgb=ray_rgb, d_counts=cnt)
        torch.cuda.synchronize()
        out[name] = (ray_rgb.cpu().numpy(), rgb.cpu().numpy(), int(cnt.item()))
    A, B = out["plain"], out["surface"]
    tol = lambda a: RTOL * np.abs(a) + ATOL_OF_MAX * np.abs(a).max()                         # noqa: E731
    print("lights: max %.4g, max abs diff %.3g, lit rays %d, shadow rays %d" % (A[0].max(), np.abs(A[0] - B[0]).max(),
                                                                                 (A[0].max(axis=1) > 0).sum(), A[2]))
    assert A[2] == B[2] == 2 * t.hit.sum() and (A[0].max(axis=1) > 0).sum() > 1000
    assert (np.abs(A[0] - B[0]) <= tol(A[0])).all() and (np.abs(A[1] - B[1]) <= tol(A[1])).all()
    # one point light through the shadow batch; rays on the floor that the small sphere shades
    lt = Yard.LIGHTS[0]
    C0 = _chain(s, t, lt)
    C1 = _chain(s, t, lt, (color, normal))
    floor = t.hit & ((t.prim & PLANE_BIT) != 0)
    shaded = floor & (C0.max(axis=1) == 0)
    print("accumulate: max %.4g, max abs diff %.3g, floor rays in shadow %d" % (C0.max(), np.abs(C0 - C1).max(), shaded.sum()))
    assert shaded.sum() > 10 and (C1[shaded] == 0).all()
    assert (np.abs(C0 - C1) <= tol(C0)).all() and (C0.max(axis=1) > 0).sum() > 1000


FLOOR_LIGHT = dict(position=(2.0, 4.5, -4.0), color=(1.0, 1.0, 1.0), wattage=30.0)       # assignment1.cpp:197-200
# a TexturedPhong's m_diffuse is what the constructor makes of kd = 1 (Texture.cpp:513-514): with ks = kt = 0, 1 -- whatever is set
FLOOR_MATERIAL = ((1.0, 1.0, 1.0), (0, 0, 0), (0, 0, 0), 20.0, 1.0)


def _stone_floor(miro, occluder=False):
    """The floor of assignment1.cpp:229-233: a plane at y = -0.5 with TexturedPhong(new StoneTexture(3), ks = 0)"""
    s = miro.Scene(0)
    s.add_triangle([40, 0, 40, 41, 0, 40, 40, 1, 40], [0, 0, 1] * 3)     # far away: a scene needs one bounded object
    if occluder:
        s.add_sphere((1.0, 1.5, -2.0), 0.8)
    s.add_plane((0, 1, 0), (0, -0.5, 0), 0)
    s.build(4)
    s.set_materials([FLOOR_MATERIAL, ((0.5, 0.5, 0.5), (0, 0, 0), (0, 0, 0), 20.0, 1.0)], [1, 1] if occluder else [1])
    s.set_textures([dict(stone=3.0)], [0, NONE])
    s.set_lights([FLOOR_LIGHT])
    return s


def _floor_rays(miro, n, seed=9):
    rng = np.random.default_rng(seed)
    o = np.stack([rng.uniform(-1, 1, n), rng.uniform(2, 4, n), rng.uniform(-1, 1, n)], 1)
    tgt = np.stack([rng.uniform(-6, 6, n), np.full(n, -0.5), rng.uniform(-8, 4, n)], 1)
    d = tgt - o
    d /= np.linalg.norm(d, axis=1)[:, None]
    rays = np.zeros(n, miro.RAY_DTYPE)
    for k, name in enumerate(("ox", "oy", "oz")):
        rays[name] = o[:, k]
    for k, name in enumerate(("dx", "dy", "dz")):
        rays[name] = d[:, k]
    rays["tmin"], rays["tmax"] = 1e-4, 1e30
    return rays


def restate_point_light(P, N, d, colour, mt, light):
    """Phong.cpp:78-156 for a point light that nothing occludes, in float32: N and the diffuse colour are given"""
    pos, col, watt = np.asarray(light["position"], F), np.asarray(light["color"], F), F(light["wattage"])
    l = (pos[None, :] - P).astype(F)
    falloff = dot3(l, l)
    l = (l * (F(1) / np.sqrt(falloff))[:, None]).astype(F)
    nDotL = dot3(N, l)
    f2 = (F(1) / (falloff * F(4) * PI * PI)).astype(F)
    diff = np.maximum(F(0), nDotL * f2 * watt).astype(F)
    kd = np.asarray(mt[0], F)
    out = (col[None, :] * (diff[:, None] * colour * kd[None, :])).astype(F)
    two = (F(2) * dot3(l, N)).astype(F)
    rv = (-l + two[:, None] * N).astype(F)
    e = dot3((-d).astype(F), rv)
    edr = np.power(np.maximum(F(0), np.minimum(F(1), e)), F(500)).astype(F)
    high = np.maximum(F(0), edr * f2 * watt).astype(F)
    return (out * F(1) + high[:, None]).astype(F)


@pytest.mark.gpu
def test_stone_floor_under_a_point_light(miro):
    """mr_shade_lights_surface on the stone floor, no occluder: ray_rgb against a float32 restatement of the Phong terms that
    takes the device's own colour and normal buffers as inputs (the test is about the shading kernel), RTOL / ATOL_OF_MAX.  The
    bump-mapped normal shows: shading with the plane's own normal differs by far more.  With an opaque sphere over the floor the
    shadowed rays are 0 and the others keep their value."""
    import torch
    s = _stone_floor(miro)
    t = Traced(miro, s, _floor_rays(miro, N_BATCH))
    color, normal, undefined = t.surface(s)
    ray_rgb = torch.zeros((t.n, 3), dtype=torch.float32, device="cuda")
    s.shade_lights_surface(t.rays, t.hits, color, normal, t.n, d_ray_rgb=ray_rgb)
    torch.cuda.synchronize()
    got = ray_rgb.cpu().numpy()
    floor = t.hit & ((t.prim & PLANE_BIT) != 0)
    assert floor.sum() == t.n and undefined == 0
    d = np.stack([t.rays_np["dx"], t.rays_np["dy"], t.rays_np["dz"]], 1).astype(F)
    c, nrm = color.cpu().numpy(), normal.cpu().numpy()
    want = restate_point_light(t.P, nrm, d, c, FLOOR_MATERIAL, FLOOR_LIGHT)
    flat = restate_point_light(t.P, np.tile(np.array([[0, 1, 0]], F), (t.n, 1)), d, c, FLOOR_MATERIAL, FLOOR_LIGHT)
    err = np.abs(got - want)
    print("stone floor: max %.4g, max abs err %.3g, lit %d, |bumped - flat| up to %.3g" % (want.max(), err.max(), (want.max(axis=1) > 0).sum(),
                                                                                            np.abs(want - flat).max()))
    assert (want.max(axis=1) > 0).sum() > 3000
    assert (err <= RTOL * np.abs(want) + ATOL_OF_MAX * want.max()).all()
    assert np.abs(want - flat).max() > 0.05 * want.max()
    # an opaque occluder
    s2 = _stone_floor(miro, occluder=True)
    t2 = Traced(miro, s2, t.rays_np)
    on_floor = t2.hit & ((t2.prim & PLANE_BIT) != 0)
    color2, normal2, _ = t2.surface(s2)
    ray_rgb2 = torch.zeros((t.n, 3), dtype=torch.float32, device="cuda")
    cnt = torch.zeros(1, dtype=torch.int64, device="cuda")
    s2.shade_lights_surface(t2.rays, t2.hits, color2, normal2, t.n, d_ray_rgb=ray_rgb2, d_counts=cnt)
    torch.cuda.synchronize()
    got2 = ray_rgb2.cpu().numpy()
    dark = on_floor & (got2.max(axis=1) == 0) & (got.max(axis=1) > 0)
    same = on_floor & ~dark
    print("with the sphere: floor rays %d, in its shadow %d" % (on_floor.sum(), dark.sum()))
    assert dark.sum() > 20 and int(cnt.item()) == t2.hit.sum()
    assert got2[same].tobytes() == got[same].tobytes()


@pytest.mark.gpu
def test_refusals_on_a_stone_scene(miro):
    """mr_shade_lights, mr_shade_accumulate, mr_shade_square_lights and mr_gen_path_rays with MR_PATH_DIFFUSE: MR_ERR_STATE on a
    scene whose table holds a STONE (or STEM) texture, the message naming the _surface calls; they work once it is cleared, and
    mr_gen_path_rays without MR_PATH_DIFFUSE works throughout."""
    import torch
    from miro_amd import binding
    s = _stone_floor(miro)
    t = Traced(miro, s, _floor_rays(miro, 515))
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

    for tex in (dict(stone=3.0), dict(stem=3.0)):
        s.set_textures([tex], [0, NONE])
        for name, call in calls():
            with pytest.raises(miro.MiroError) as e:
                call()
            assert e.value.status == -5 and name in str(e.value) and "_surface" in str(e.value), (name, str(e.value))
        path(binding.MR_PATH_MIRROR | binding.MR_PATH_REFRACT)()
    s.set_textures([])
    for name, call in calls():
        call()
    torch.cuda.synchronize()
    assert float(rgb.max()) > 0


STONE_FRAME = dict(eye=(0.0, 3.0, 6.0), lookat=(0.0, -0.5, -3.0), up=(0.0, 1.0, 0.0), fov=45.0, light=FLOOR_LIGHT["position"],
                   wattage=FLOOR_LIGHT["wattage"])


@pytest.mark.gpu
def test_stone_floor_frame_through_render_specular(miro):
    """32 x 32, 1 spp, depth 0: FrameRenderer.render_specular on the stone floor equals trace -> mr_hit_surface ->
    mr_shade_lights_surface driven by hand, byte for byte, in the light-list form; the single-light form (shadow batch ->
    mr_shade_accumulate_surface) gives the same frame within RTOL / ATOL_OF_MAX."""
    import torch
    from miro_amd import frame
    s = _stone_floor(miro)
    W = H = 32
    fr = frame.FrameRenderer(s, STONE_FRAME, W, H, spp=1)
    fr.generate()
    per_level = fr.render_specular(depth=0, lights=[FLOOR_LIGHT])
    torch.cuda.synchronize()
    got = fr.d_rgb.cpu().numpy().copy()
    n = W * H
    assert per_level[0][0] == n and per_level[0][1] > n // 2
    f32 = dict(dtype=torch.float32, device="cuda")
    hits, color, normal, rgb = torch.empty((n, 4), **f32), torch.empty((n, 3), **f32), torch.empty((n, 3), **f32), torch.zeros((n, 3), **f32)
    s.trace_device(fr.d_rays, n, hits)
    s.hit_surface(fr.d_rays, hits, n, color, normal)
    s.shade_lights_surface(fr.d_rays, hits, color, normal, n, rgb)
    torch.cuda.synchronize()
    want = rgb.cpu().numpy()
    assert want.max() > 0 and (want.max(axis=1) > 0).sum() > n // 2
    assert got.tobytes() == want.tobytes()
    fr.render_specular(depth=0)                                          # the description's single point light
    torch.cuda.synchronize()
    single = fr.d_rgb.cpu().numpy()
    assert (np.abs(single - want) <= RTOL * np.abs(want) + ATOL_OF_MAX * want.max()).all()
