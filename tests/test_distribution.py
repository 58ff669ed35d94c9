"""mr_gen_eye_rays_lens / mr_shade_square_lights (csrc/mr_distribution.hip) -- the thin-lens camera (Camera.cpp:135-160 under
-DDOF, sampleDisc Utility.h:82-95) and Phong::shade over SquareLights (SquareLight.h:6-58, Phong.cpp:66-157).

The checkers are restatements written here in numpy float32, one operation per rounding, from the cited lines of the
reference; they import nothing from the product but its already-verified entry points: mr_trace for the shadow hits and
mr_hit_attrs for P / N (the oracle cannot grow).  The plain-camera half of the lens restatement (frame, pixel hash, jitter)
is held to the oracle's eye rays on the CPU.

Which comparison applied to the lens rays: BIT EQUALITY (the library is built without contraction; tests/test_gpu_parity.py
compares generated eye rays by their bytes, so there is no tolerance to fall back to).  The square light is compared at the
tolerance tests/test_lights.py applies to mr_shade_lights against its checker (rtol 1e-5, atol 1e-7 x max: powf on the device
vs pow in the checker needs it)."""
import ctypes as C
import math
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
MISS = 0xFFFFFFFF
RTOL, ATOL_OF_MAX = 1e-5, 1e-7                                  # tests/test_lights.py:25
M32 = np.uint64(0xFFFFFFFF)
LENS_ROUNDS, LENS_DOMAIN, SQUARE_DOMAIN = 32, 0x4c454e53, 0x73717561

CAMERA = dict(eye=(0.0, 3.0, 6.0), lookat=(0.0, 0.0, 0.0), up=(0.0, 1.0, 0.0), fov=45.0)       # the teapot fixture's
LENS_W = LENS_H = 8
LENS_SPP, APERTURE, LENS_SEED = 4, 0.2, 168


# ---- the restatements ----------------------------------------------------------------------------------------------------
def pcg(x):
    """pcg32 of uint32 values (held in uint64 so that the products do not overflow numpy's integers)"""
    x = np.asarray(x, np.uint64) & M32
    state = (x * np.uint64(747796405) + np.uint64(2891336453)) & M32
    word = (((state >> ((state >> np.uint64(28)) + np.uint64(4))) ^ state) * np.uint64(277803737)) & M32
    return (word >> np.uint64(22)) ^ word


def unit01(h):
    return (h >> np.uint64(8)).astype(F) * F(1.0 / 16777216.0)


def dot3(a, b):
    return (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]


def cross(a, b):
    return np.array([a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]], F)


def unit(a):
    inv = F(1) / np.sqrt((a[0] * a[0] + a[1] * a[1]) + a[2] * a[2])
    return (a * inv).astype(F)


def normalised_rows(N):
    return (N * (F(1) / np.sqrt(dot3(N, N)))[:, None]).astype(F)


def frame_of(cam, W, H):
    """Camera.h:79-110, Camera.cpp:113-124"""
    eye, lookat, up = (np.asarray(cam[k], F) for k in ("eye", "lookat", "up"))
    f = dict(eye=eye, view=unit((lookat - eye).astype(F)))
    f["w"] = unit(-f["view"])
    f["u"] = unit(cross(unit(up), f["w"]))
    f["v"] = cross(f["w"], f["u"])
    half_deg = (PI / F(180.0)) / F(2.0)
    f["top"] = F(math.tan(float(F(cam["fov"]) * half_deg)))
    f["right"] = (F(W) / F(H)) * f["top"]
    f["bottom"], f["left"] = -f["top"], -f["right"]
    return f


def sample_indices(W, H, spp):
    k = np.arange(W * H * spp, dtype=np.uint64)
    pix, sm = k // np.uint64(spp), k % np.uint64(spp)
    return pix % np.uint64(W), pix // np.uint64(W), sm


def sample_hash(W, H, spp, seed):
    x, y, sm = sample_indices(W, H, spp)
    return pcg(pcg(pcg(np.uint64(seed)) ^ (y * np.uint64(W) + x)) + sm)


def jitter_of(h):
    return unit01(pcg(h)), unit01(pcg(h ^ np.uint64(0x68bc21eb)))


def lens_samples_of(h, aperture):
    """sampleDisc (Utility.h:82-95) over the documented keys: (lx, ly, rounds used; LENS_ROUNDS + 1 = exhausted)"""
    a = F(aperture)
    lx, ly = np.zeros(len(h), F), np.zeros(len(h), F)
    used = np.full(len(h), LENS_ROUNDS + 1)
    for r in range(LENS_ROUNDS):
        fx = unit01(pcg(h ^ np.uint64(LENS_DOMAIN + 2 * r)))
        fy = unit01(pcg(h ^ np.uint64(LENS_DOMAIN + 2 * r + 1)))
        xr, yr = (F(2) * fx - F(1)) * a, (F(2) * fy - F(1)) * a
        take = (used > LENS_ROUNDS) & ~(xr * xr + yr * yr > a * a)
        lx[take], ly[take], used[take] = xr[take], yr[take], r + 1
    return lx, ly, used


def restate_eye_rays(cam, W, H, spp, samples, lens=None):
    """Camera::eyeRay (Camera.cpp:127-160) for samples [n, 4] = dx, dy, lx, ly; lens = (aperture, focus_plane) or None for the
    #else branch (new_eye = eye, localwDir = wDir).  Returns [n, 8] float32."""
    f = frame_of(cam, W, H)
    x, y, _ = sample_indices(W, H, spp)
    dx, dy, lx, ly = (samples[:, c] for c in range(4))
    upos = f["left"] + (f["right"] - f["left"]) * ((x.astype(F) + dx) / F(W))
    vpos = f["bottom"] + (f["top"] - f["bottom"]) * ((y.astype(F) + dy) / F(H))
    n = len(x)
    out = np.zeros((n, 8), F)
    if lens is None:
        e = np.repeat(f["eye"][None, :], n, axis=0)
        lw = np.repeat(f["w"][None, :], n, axis=0)
    else:
        focus = (f["eye"] + f["view"] * F(lens[1])).astype(F)                                  # :142
        e = np.stack([f["eye"][c] + (lx * f["u"][c] + ly * f["v"][c]) for c in range(3)], 1).astype(F)   # :140
        lw = normalised_rows((-(focus[None, :] - e)).astype(F))                                # :142, :145
    d = np.stack([(upos * f["u"][c] + vpos * f["v"][c]) - lw[:, c] for c in range(3)], 1).astype(F)      # :160
    out[:, 0:3], out[:, 4:7], out[:, 7] = e, normalised_rows(d), F(1e12)
    return out


def tangents_np(normal):
    """getTangents (Utility.h:25-31)"""
    n = np.asarray(normal, F)
    t1 = cross(np.array([0, 0, 1], F), n)
    if float((t1[0] * t1[0] + t1[1] * t1[1]) + t1[2] * t1[2]) < 1e-6:
        t1 = cross(np.array([0, 1, 0], F), n)
    return t1, cross(t1, n)


def rays_of(dtype, o, d, tmax):
    r = np.zeros(len(o), dtype)
    r["ox"], r["oy"], r["oz"], r["tmin"] = o[:, 0], o[:, 1], o[:, 2], 0.0
    r["dx"], r["dy"], r["dz"], r["tmax"] = d[:, 0], d[:, 1], d[:, 2], tmax
    return r


# ---- the square-light scene: a floor of two triangles, one small occluder above it; variant: a glass sphere ------------------
FLOOR_Y, HALF = 0.0, 1.4
OCCLUDER = [(-0.7, 1.0, -0.55), (0.7, 1.0, -0.55), (0.0, 1.0, 0.75)]
SPHERE = ((0.85, 0.45, 0.35), 0.33)
#            diffuse            specular           transmission       shininess  index
MATERIALS = [((0.8, 0.7, 0.6), (0.0, 0.0, 0.0), (0.0, 0.0, 0.0), 20.0, 1.0),                  # floor: a highlight (pow(., 500))
             ((0.3, 0.6, 0.9), (0.0, 0.0, 0.0), (0.0, 0.0, 0.0), float("inf"), 1.0),          # occluder: no highlight
             ((0.1, 0.1, 0.1), (0.1, 0.1, 0.1), (0.8, 0.8, 0.8), 50.0, 1.5)]                  # glass
SQ_CAMERA = dict(eye=(0.0, 5.0, 3.0), lookat=(0.0, 0.0, 0.0), up=(0.0, 1.0, 0.0), fov=30.0)
SQ_W = SQ_H = 16
LIGHT_A = dict(position=(0.0, 3.0, 0.0), normal=(0.0, -1.0, 0.0), color=(1.0, 0.9, 0.8), wattage=120.0, dimensions=(0.9, 0.9))
LIGHT_B = dict(position=(-1.5, 2.5, 1.0), normal=(0.5, -1.0, 0.25), color=(0.3, 0.5, 1.0), wattage=60.0, dimensions=(0.8, 0.4))


def material_table():
    """11 floats per material as the Phong constructor leaves them (Phong.cpp:12-33)"""
    rows = []
    for kd, ks, kt, sh, ri in MATERIALS:
        ks, kt, kd = np.asarray(ks, F), np.asarray(kt, F), np.asarray(kd, F)
        kt = np.maximum(np.minimum(kt, F(1.0) - ks), F(0))
        kd = np.maximum(np.minimum(kd, F(1.0) - ks - kt), F(0))
        rows.append(list(kd) + list(ks) + list(kt) + [sh, ri])
    return np.array(rows, F)


class SquareScene:
    """The product scene with its primary batch traced, and what the checker needs of it, computed once."""

    def __init__(self, miro, sphere):
        import torch
        from miro_amd import binding
        self.miro, self.torch = miro, torch
        s = miro.Scene(0)
        up = [0, 1, 0] * 3
        a, b = -HALF, HALF
        s.add_triangle([a, FLOOR_Y, a, a, FLOOR_Y, b, b, FLOOR_Y, b], up)
        s.add_triangle([a, FLOOR_Y, a, b, FLOOR_Y, b, b, FLOOR_Y, a], up)
        s.add_triangle([c for v in OCCLUDER for c in v], up)
        prim_mat = [0, 0, 1]
        if sphere:
            s.add_sphere(*SPHERE)
            prim_mat.append(2)
        s.set_materials(MATERIALS if sphere else MATERIALS[:2], prim_mat)             # no refractive material without the sphere
        s.build(4)
        self.scene, self.prim_mat, self.mats = s, np.asarray(prim_mat, np.uint32), material_table()
        self.n = SQ_W * SQ_H
        self.d_rays = torch.empty((self.n, 8), dtype=torch.float32, device="cuda")
        self.d_hits = torch.empty((self.n, 4), dtype=torch.float32, device="cuda")
        s.gen_eye_rays(binding.make_camera(SQ_CAMERA["eye"], SQ_CAMERA["lookat"], SQ_CAMERA["up"], SQ_CAMERA["fov"]), SQ_W, SQ_H, self.d_rays)
        s.trace_device(self.d_rays, self.n, self.d_hits)
        torch.cuda.synchronize()
        self.rays = self.d_rays.cpu().numpy().view(miro.RAY_DTYPE).reshape(-1)
        self.hits = self.d_hits.cpu().numpy().view(miro.HIT_DTYPE).reshape(-1)
        self.idx = np.nonzero(self.hits["prim"] != MISS)[0]
        P, N = self.attrs(self.rays[self.idx], self.hits[self.idx])
        self.P, self.N = P, normalised_rows(N)                                                  # Scene.cpp:262
        self._checked, self.through = {}, {}                                                    # through: samples scaled by dot(N, l)

    def attrs(self, rays, hits):
        """mr_hit_attrs for host records: (P, N as HitInfo holds it)"""
        torch = self.torch
        n = len(rays)
        dr = torch.from_numpy(np.ascontiguousarray(rays).view(F).reshape(n, 8).copy()).cuda()
        dh = torch.from_numpy(np.ascontiguousarray(hits).view(F).reshape(n, 4).copy()).cuda()
        dP, dN = torch.empty((n, 3), dtype=torch.float32, device="cuda"), torch.empty((n, 3), dtype=torch.float32, device="cuda")
        self.scene.hit_attrs(dh, n, dP, dN, d_rays=dr)
        torch.cuda.synchronize()
        return dP.cpu().numpy(), dN.cpu().numpy()

    def uv(self, n_lights, samples):
        """seeded pairs in [0, 1), exactly representable: [n, lights, samples, 2]"""
        rng = np.random.RandomState(1000 * n_lights + samples)
        return (rng.randint(0, 1 << 24, size=(self.n, n_lights, samples, 2)).astype(F) * F(1.0 / 16777216.0)).astype(F)

    def restate(self, lights, samples, uv):
        """Phong::shade (Phong.cpp:66-157) over SquareLights for the batch: (L [n, 3], occluded samples per ray and light
        [n, lights], fragile rays)"""
        key = (len(lights), samples)
        if key in self._checked:
            return self._checked[key]
        idx, P, N = self.idx, self.P, self.N
        m = len(idx)
        L = np.zeros((m, 3), F)
        blocked = np.zeros((m, len(lights)), np.int64)
        fragile = np.zeros(m, bool)
        n_through = 0
        r = self.rays[idx]
        e = -np.stack([r["dx"], r["dy"], r["dz"]], 1).astype(F)                                 # :49
        mt = self.mats[self.prim_mat[self.hits["prim"][idx]]]
        shiny = mt[:, 9] < np.inf
        fs = F(samples)
        for j, lt in enumerate(lights):
            pos, color, watt = np.asarray(lt["position"], F), np.asarray(lt["color"], F), F(lt["wattage"])
            t1, t2 = tangents_np(lt["normal"])                                                  # SquareLight::preCalc
            dims = np.asarray(lt["dimensions"], F)
            side_length = np.sqrt(F(samples))                                                   # SquareLight.h:27-29
            du, dv = dims[0] / side_length, dims[1] / side_length
            for i in range(samples):
                sx, sy = i % int(side_length), i // int(side_length)                            # :32-33
                u = ((du * uv[idx, j, i, 0]) + F(sx) * du) - dims[0] / F(2.0)                   # :35-36
                v = ((dv * uv[idx, j, i, 1]) + F(sy) * dv) - dims[1] / F(2.0)
                origin = np.stack([(pos[c] + u * t1[c]) + v * t2[c] for c in range(3)], 1).astype(F)       # :38
                l = (origin - P).astype(F)                                                      # PointLight.h:42
                falloff = dot3(l, l)                                                            # Phong.cpp:85
                length = np.sqrt(falloff)
                l = (l * (F(1) / length)[:, None]).astype(F)                                    # :88
                sr = rays_of(self.miro.RAY_DTYPE, (P + l * EPS).astype(F), l, length)           # :92
                sh = self.scene.trace(sr)                                                       # :97, closest hit
                intensity = np.ones(m, F)
                skip = np.zeros(m, bool)
                occ = np.nonzero(sh["prim"] != MISS)[0]
                if len(occ):
                    om = self.mats[self.prim_mat[sh["prim"][occ]]]
                    refr = (om[:, 6] > 0) | (om[:, 7] > 0) | (om[:, 8] > 0)                     # :99
                    _, Ns = self.attrs(sr[occ], sh[occ])
                    dn = dot3(normalised_rows(Ns), l[occ])                                      # :102-111
                    through = refr & ~(dn < 0) & ~(dn < EPS)
                    intensity[occ[through]] = dn[through]
                    n_through += int(through.sum())
                    skip[occ[~through]] = True
                    fragile[occ[refr & ((np.abs(dn) <= 1e-6) | (np.abs(dn - EPS) <= 1e-6))]] = True
                blocked[:, j] += skip
                nDotL = dot3(N, l)                                                              # :139
                f2 = F(1.0) / (falloff * F(4.0) * PI * PI)                                      # :140
                diff = np.maximum(F(0), nDotL * f2 * watt / fs)                                 # :146
                term = (color[None, :] * (diff[:, None] * mt[:, 0:3] * mt[:, 0:3]) * intensity[:, None]).astype(F)
                two = 2 * dot3(l, N)
                rv = (-l + two[:, None] * N).astype(F)                                          # :151
                edr = np.power(np.maximum(F(0), np.minimum(F(1), dot3(e, rv))), F(500)).astype(F)          # :152
                high = np.where(shiny, np.maximum(F(0), edr * f2 * watt / fs), F(0)).astype(F)  # :154
                keep = ~skip
                L[keep] = (L[keep] + term[keep]).astype(F)                                      # :146, then :155
                L[keep] = (L[keep] + high[keep, None]).astype(F)
        full = np.zeros((self.n, 3), F)
        full[idx] = L
        blocked_full = np.zeros((self.n, len(lights)), np.int64)
        blocked_full[idx] = blocked
        fragile_full = np.zeros(self.n, bool)
        fragile_full[idx] = fragile
        self._checked[key] = (full, blocked_full, fragile_full)
        self.through[key] = n_through
        return self._checked[key]

    def shade(self, lights, samples, uv=None, seed=168, weights=None, pixels=None, spp=1, n_pixels=None, flags=0):
        """(d_rgb, d_ray_rgb, shadow rays) of mr_shade_square_lights as numpy"""
        torch = self.torch
        n = self.n
        rgb = torch.zeros((n // spp if n_pixels is None else n_pixels, 3), dtype=torch.float32, device="cuda")
        ray_rgb = torch.full((n + 1, 3), -7.0, dtype=torch.float32, device="cuda")             # one sentinel row after the end
        cnt = torch.zeros(1, dtype=torch.int64, device="cuda")
        d_uv = torch.from_numpy(uv).cuda() if uv is not None else None
        self.scene.shade_square_lights(lights, samples, self.d_rays, self.d_hits, n, rgb, seed=seed, d_weights=weights, d_pixels=pixels,
                                       d_uv_in=d_uv, spp=spp, flags=flags, d_ray_rgb=ray_rgb, d_counts=cnt)
        torch.cuda.synchronize()
        out = ray_rgb.cpu().numpy()
        assert (out[n] == -7.0).all(), "d_ray_rgb was written beyond 3n floats"
        return rgb.cpu().numpy(), out[:n].copy(), int(cnt.item())


@pytest.fixture(scope="module")
def plain(miro):
    return SquareScene(miro, sphere=False)


@pytest.fixture(scope="module")
def glass(miro):
    return SquareScene(miro, sphere=True)


# ---- without a GPU -------------------------------------------------------------------------------------------------------
def host_scene(miro):
    s = miro.Scene()
    s.add_triangle([0, 0, 0, 1, 0, 0, 0, 1, 0], [0, 0, 1] * 3)
    s.build(4, host_only=True)
    return s


def test_the_distribution_entries_are_exported_and_declared(miro, tmp_path):
    from miro_amd import binding
    L = miro.lib()
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "miro_hip.h")).read(), flags=re.S)
    for name in ("mr_gen_eye_rays_lens", "mr_shade_square_lights", "mr_square_light_tangents"):
        assert hasattr(L, name) and name in miro.EXPORTED_SYMBOLS and re.search(r"\b%s\s*\(" % name, src), name
    prog = ('#include "miro_hip.h"\n#include <stdio.h>\nint main(void) { printf("%d %d\\n", (int)sizeof(mr_lens_desc), '
            '(int)sizeof(mr_square_light_desc)); return 0; }\n')
    exe = str(tmp_path / "sizeof_distribution")
    subprocess.run(["gcc", "-x", "c", "-", "-I", os.path.join(ROOT, "include"), "-o", exe], input=prog.encode(), check=True)
    assert subprocess.check_output([exe]).split() == [b"%d" % C.sizeof(binding.LensDesc), b"%d" % C.sizeof(binding.SquareLightDesc)] == [b"32", b"64"]


def test_lens_argument_errors(miro):
    """Every listed error: MR_ERR_INVALID with a message, before any device call (no device is present here)."""
    from miro_amd import binding
    L = miro.lib()
    s = host_scene(miro)
    cam = binding.make_camera(CAMERA["eye"], CAMERA["lookat"], CAMERA["up"], CAMERA["fov"])
    dummy = C.c_void_p(64)

    def lens(aperture=0.2, focus_plane=5.0, reserved=(0,) * 6):
        d = binding.LensDesc()
        d.aperture, d.focus_plane = aperture, focus_plane
        d.reserved[:] = reserved
        return d

    def call(ln, scene=s.h, rays=dummy, window=(8, 8, 0, 8, 4), s_in=None):
        W, H, y0, y1, spp = window
        return L.mr_gen_eye_rays_lens(scene, C.byref(cam), W, H, y0, y1, spp, 1, 168, rays, None, C.byref(ln) if ln is not None else None,
                                      s_in, None, None)

    inf, nan = float("inf"), float("nan")
    assert call(None) == -1 and b"lens" in L.mr_last_error()
    for bad, word in ((lens(reserved=(0, 0, 0, 0, 0, 1)), b"reserved"), (lens(aperture=-0.1), b"aperture"), (lens(aperture=nan), b"aperture"),
                      (lens(aperture=inf), b"aperture"), (lens(focus_plane=0.0), b"focus_plane"), (lens(focus_plane=-1.0), b"focus_plane"),
                      (lens(focus_plane=inf), b"focus_plane"), (lens(focus_plane=nan), b"focus_plane")):
        assert call(bad) == -1, word
        assert word in L.mr_last_error(), (word, L.mr_last_error())
    ok = lens(aperture=0.0)                                                                   # a pinhole is a legal lens
    assert call(ok, scene=None) == -1 and call(ok, rays=None) == -1
    assert call(ok, window=(8, 8, 4, 2, 4)) == -1 and call(ok, window=(8, 8, 0, 9, 4)) == -1 and call(ok, window=(8, 8, 0, 8, 0)) == -1
    assert call(ok, rays=C.c_void_p(8)) == -1 and call(ok, s_in=C.c_void_p(8)) == -1 and b"aligned" in L.mr_last_error()


def test_square_light_argument_errors(miro):
    """Every listed error: MR_ERR_INVALID before the scene's state is looked at; a valid call on a host_only or unbuilt scene:
    MR_ERR_STATE, never a CPU path."""
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

    def call(lights, n_lights, samples=4, scene=s.h, rays=dummy, hits=dummy, rgb=dummy, spp=1, flags=0, n=4, uv=None):
        return L.mr_shade_square_lights(scene, lights, n_lights, samples, 168, rays, hits, None, None, uv, n, spp, flags, rgb, None, None, None)

    inf, nan = float("inf"), float("nan")
    ok = light()
    assert call(arr(ok), 1, scene=None) == -1 and b"NULL" in L.mr_last_error()
    assert call(None, 1) == -1 and b"NULL" in L.mr_last_error()
    assert call(arr(ok), 0) == -1 and call(arr(*[ok] * 9), 9) == -1 and b"at most" in L.mr_last_error()
    for bad, word in ((light(reserved=(0, 1, 0, 0)), b"reserved"), (light(position=(0, nan, 0)), b"finite"), (light(color=(inf, 1, 1)), b"finite"),
                      (light(wattage=nan), b"finite"), (light(normal=(0, 0, 0)), b"normal"), (light(normal=(0, nan, 0)), b"normal"),
                      (light(dimensions=(-1.0, 1.0)), b"dimensions"), (light(dimensions=(1.0, inf)), b"dimensions"),
                      (light(dimensions=(nan, 1.0)), b"dimensions")):
        assert call(arr(ok, bad), 2) == -1, word
        assert word in L.mr_last_error(), (word, L.mr_last_error())
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


@pytest.mark.parametrize("normal", [(0.0, -1.0, 0.0), (0.5, -1.0, 0.25), (0.0, 0.0, 1.0), (0.0, 0.0, -2.5), (3e-4, 4e-4, 1.0),
                                    (1e-3, 0.0, 1.0), (0.3, 0.2, -0.1)])
def test_host_tangents_are_getTangents(miro, normal):
    """mr_square_light_tangents against the numpy restatement of Utility.h:25-31, bit for bit, for normals that do ((0, 0, z),
    and x^2 + y^2 < 1e-6) and do not take the `t1.length2() < 1e-6` branch."""
    from miro_amd import binding
    t1, t2 = binding.square_light_tangents(normal)
    w1, w2 = tangents_np(normal)
    n = np.asarray(normal, F)
    first = cross(np.array([0, 0, 1], F), n)
    took_branch = float(dot3(first[None, :], first[None, :])[0]) < 1e-6
    assert took_branch == (normal[0] ** 2 + normal[1] ** 2 < 1e-6)
    assert t1.tobytes() == w1.tobytes() and t2.tobytes() == w2.tobytes()
    assert abs(float(np.dot(w1.astype(np.float64), n))) < 1e-6 and abs(float(np.dot(w2.astype(np.float64), n))) < 1e-6
    assert np.any(w1 != 0) and np.any(w2 != 0)


@pytest.mark.parametrize("cam,W,H,spp", [(CAMERA, LENS_W, LENS_H, LENS_SPP), (SQ_CAMERA, SQ_W, SQ_H, 1), (CAMERA, 37, 23, 3)])
def test_plain_half_of_the_lens_restatement_is_the_oracles_eye_ray(oracle, cam, W, H, spp):
    """The frame, the per-sample hash and the jitter of the restatement, through its #else branch (no lens), give the oracle's
    eye rays bit for bit: what the lens tests add on top is Camera.cpp:138-145 alone."""
    jitter = spp > 1
    h = sample_hash(W, H, spp, LENS_SEED)
    s = np.zeros((len(h), 4), F)
    s[:, 0], s[:, 1] = jitter_of(h) if jitter else (F(0.5), F(0.5))
    want = oracle.eye_rays(oracle.make_camera(cam["eye"], cam["lookat"], cam["up"], cam["fov"]), W, H, spp=spp, jitter=jitter, seed=LENS_SEED)
    assert restate_eye_rays(cam, W, H, spp, s).tobytes() == want.tobytes()


def test_no_lens_sample_of_the_gpu_input_exhausts_the_rounds():
    """From the restated hash: every sample of the GPU tests' input is accepted within the 32 rounds (per-round acceptance
    PI / 4), inside the disc, and the rounds are really used (some sample needs more than one)."""
    for seed in (LENS_SEED, LENS_SEED + 1):
        lx, ly, used = lens_samples_of(sample_hash(LENS_W, LENS_H, LENS_SPP, seed), APERTURE)
        assert used.max() <= LENS_ROUNDS and used.max() > 1
        assert (lx * lx + ly * ly <= F(APERTURE) * F(APERTURE)).all() and np.abs(lx).max() > 0.5 * APERTURE


def test_distribution_kernels_stay_inside_the_verified_envelope():
    """Every kernel of mr_distribution.hip: no dynamic stack; no more spilled VGPRs, no more scratch per lane and no fewer waves
    per SIMD than BOTH its own record (tests/golden/kernel_budget_distribution.json, written from the build whose GPU tests were
    green) AND the worst value among the kernels of tests/golden/kernel_budget.json."""
    cur = kernel_budget.unit_kernels("mr_distribution")
    assert len(cur) == 13 and sum("shade_square_lights_kernel" in k for k in cur) == 12 and sum("eye_rays_lens_kernel" in k for k in cur) == 1
    kernel_budget.assert_inside_envelope(cur, "kernel_budget_distribution.json")


# ---- on the MI355X: the lens ---------------------------------------------------------------------------------------------
FOCUS = float(np.sqrt(np.sum(np.square(np.asarray(CAMERA["eye"], F) - np.asarray(CAMERA["lookat"], F)))))   # the camera distance


class Lens:
    def __init__(self, miro):
        import torch
        from miro_amd import binding
        self.torch = torch
        self.scene = miro.Scene(0)
        self.scene.add_triangle([-1, 0, -1, 1, 0, -1, 0, 0, 1], [0, 1, 0] * 3)
        self.scene.build(4)
        self.cam = binding.make_camera(CAMERA["eye"], CAMERA["lookat"], CAMERA["up"], CAMERA["fov"])
        self.n = LENS_W * LENS_H * LENS_SPP

    def gen(self, samples_in=None, seed=LENS_SEED, aperture=APERTURE):
        """(rays [n, 8], samples used [n, 4], counters) of one call"""
        torch = self.torch
        rays = torch.full((self.n + 1, 8), -7.0, dtype=torch.float32, device="cuda")           # one sentinel row after the end
        out = torch.full((self.n + 1, 4), -7.0, dtype=torch.float32, device="cuda")
        cnt = torch.zeros(2, dtype=torch.int64, device="cuda")
        d_in = torch.from_numpy(samples_in).cuda() if samples_in is not None else None
        got = self.scene.gen_eye_rays_lens(self.cam, LENS_W, LENS_H, rays, aperture, FOCUS, spp=LENS_SPP, jitter=True, seed=seed,
                                           d_samples_in=d_in, d_samples_out=out, d_counts=cnt)
        torch.cuda.synchronize()
        r, o = rays.cpu().numpy(), out.cpu().numpy()
        assert got == self.n and (r[self.n] == -7.0).all() and (o[self.n] == -7.0).all(), "written beyond the batch"
        return r[:self.n].copy(), o[:self.n].copy(), cnt.cpu().numpy().tolist()


@pytest.fixture(scope="module")
def lens(miro):
    return Lens(miro)


@pytest.mark.gpu
def test_lens_rays_of_explicit_samples_are_the_restatement_bit_for_bit(lens):
    """d_samples_in from seeded numpy values, lens pairs inside the disc: origins and directions equal, as uint32, the numpy
    restatement of Camera.cpp:138-160; the origins really move, by at most the aperture."""
    rng = np.random.RandomState(7)
    n = lens.n
    s = np.zeros((n, 4), F)
    s[:, 0:2] = rng.rand(n, 2).astype(F) * F(0.999)
    rad, ang = F(APERTURE) * np.sqrt(rng.rand(n)).astype(F) * F(0.999), rng.rand(n) * 2 * np.pi
    s[:, 2], s[:, 3] = (rad * np.cos(ang)).astype(F), (rad * np.sin(ang)).astype(F)
    s[0, 2:4] = 0.0                                                                           # the lens centre
    assert (s[:, 2] ** 2 + s[:, 3] ** 2 <= F(APERTURE) ** 2).all()
    want = restate_eye_rays(CAMERA, LENS_W, LENS_H, LENS_SPP, s, lens=(APERTURE, FOCUS))
    got, used, counts = lens.gen(samples_in=s)
    bad = np.nonzero((got.view(np.uint32) != want.view(np.uint32)).any(axis=1))[0]
    print("%d of %d rays differ; worst |difference| %.3g" % (len(bad), n, np.abs(got - want).max()))
    assert len(bad) == 0, (bad[:5], got[bad[:5]], want[bad[:5]])
    assert used.tobytes() == s.tobytes() and counts == [n, 0]
    eye = np.asarray(CAMERA["eye"], F)
    moved = np.linalg.norm(got[:, 0:3] - eye, axis=1)
    assert moved[0] == 0 and moved.max() > 0.5 * APERTURE and moved.max() <= APERTURE * 1.001


@pytest.mark.gpu
def test_lens_internal_samples_counters_and_seeds(lens):
    """d_samples_in NULL: the samples written to d_samples_out are the documented hash's (dx, dy those of mr_gen_eye_rays for the
    seed, every lens pair inside the disc), the rays are the restatement's for them, replaying them through d_samples_in gives
    identical bits; d_counts == [n, 0]; the same seed twice the same bits, another seed other lens samples."""
    n = lens.n
    rays, used, counts = lens.gen()
    h = sample_hash(LENS_W, LENS_H, LENS_SPP, LENS_SEED)
    dx, dy = jitter_of(h)
    lx, ly, rounds = lens_samples_of(h, APERTURE)
    assert counts == [n, 0] and rounds.max() <= LENS_ROUNDS
    assert (used[:, 2] ** 2 + used[:, 3] ** 2 <= F(APERTURE) ** 2).all()
    assert used[:, 0].tobytes() == dx.tobytes() and used[:, 1].tobytes() == dy.tobytes()     # the jitter of mr_gen_eye_rays
    assert used[:, 2].tobytes() == lx.tobytes() and used[:, 3].tobytes() == ly.tobytes()
    assert rays.tobytes() == restate_eye_rays(CAMERA, LENS_W, LENS_H, LENS_SPP, used, lens=(APERTURE, FOCUS)).tobytes()
    pinhole, used0, _ = lens.gen(aperture=0.0)                                                # aperture 0: the same jitter, no lens offset
    assert used0[:, 0:2].tobytes() == used[:, 0:2].tobytes() and (used0[:, 2:4] == 0).all()
    assert (pinhole[:, 0:3] == np.asarray(CAMERA["eye"], F)).all()
    replay, used2, _ = lens.gen(samples_in=used)
    assert replay.tobytes() == rays.tobytes() and used2.tobytes() == used.tobytes()
    again, used3, _ = lens.gen()
    assert again.tobytes() == rays.tobytes() and used3.tobytes() == used.tobytes()
    other, used4, counts4 = lens.gen(seed=LENS_SEED + 1)
    assert counts4 == [n, 0] and (used4[:, 2:4] != used[:, 2:4]).any(axis=1).mean() > 0.99


# ---- on the MI355X: the square light -------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("which", ["plain", "glass"])
def test_a_square_of_no_extent_is_the_point_light_bit_for_bit(request, which):
    """dimensions = (0, 0), samples = 1: d_ray_rgb equals, as uint32, mr_shade_lights' with one MR_LIGHT_POINT at the same
    position -- on the triangle scene and on the one with the glass sphere (the Phong.cpp:99-113 arm, the objects variant)."""
    sc = request.getfixturevalue(which)
    torch = sc.torch
    sq = dict(LIGHT_A, dimensions=(0.0, 0.0))
    _, got, counted = sc.shade([sq], 1)
    sc.scene.set_lights([dict(position=LIGHT_A["position"], color=LIGHT_A["color"], wattage=LIGHT_A["wattage"])])
    want = torch.zeros((sc.n, 3), dtype=torch.float32, device="cuda")
    cnt = torch.zeros(1, dtype=torch.int64, device="cuda")
    sc.scene.shade_lights(sc.d_rays, sc.d_hits, sc.n, None, d_ray_rgb=want, d_counts=cnt)
    torch.cuda.synchronize()
    want = want.cpu().numpy()
    assert want.max() > 0 and counted == int(cnt.item()) == len(sc.idx) and 0 < len(sc.idx) < sc.n
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert (want[sc.idx] == 0).all(axis=1).any() and (want[sc.idx] > 0).all(axis=1).any()      # shadowed and lit hits


@pytest.mark.gpu
@pytest.mark.parametrize("samples", [1, 4, 49])
@pytest.mark.parametrize("n_lights", [1, 2])
def test_square_lights_of_explicit_pairs_match_the_restatement(plain, samples, n_lights):
    """d_ray_rgb against the numpy restatement of SquareLight.h:23-39 and Phong.cpp:78-156 whose shadow rays mr_trace traces, at
    the tolerance of tests/test_lights.py; d_counts[0] == hits x lights x samples.  At 49 samples the checker alone shows that
    the batch holds umbra (every sample of light A occluded), penumbra (a strict subset) and lit (none) rays."""
    lights = [LIGHT_A, LIGHT_B][:n_lights]
    uv = plain.uv(n_lights, samples)
    want, blocked, fragile = plain.restate(lights, samples, uv)
    _, got, counted = plain.shade(lights, samples, uv=uv)
    hit = plain.hits["prim"] != MISS
    scale = float(want.max())
    err = np.abs(got.astype(np.float64) - want) - RTOL * np.abs(want)
    regions = dict(umbra=int((hit & (blocked[:, 0] == samples)).sum()), lit=int((hit & (blocked[:, 0] == 0)).sum()),
                   penumbra=int((hit & (blocked[:, 0] > 0) & (blocked[:, 0] < samples)).sum()))
    print("samples %d, lights %d: %d hits of %d, scale %.4g, worst excess over rtol %.3g (atol %.3g), regions %s" % (
        samples, n_lights, hit.sum(), plain.n, scale, err.max(), ATOL_OF_MAX * scale, regions))
    assert counted == int(hit.sum()) * n_lights * samples and 0 < hit.sum() < plain.n
    assert scale > 0 and not fragile.any()
    assert regions["umbra"] > 0 and regions["lit"] > 0
    if samples == 49:
        assert regions["penumbra"] > 0
    assert np.allclose(got, want, rtol=RTOL, atol=ATOL_OF_MAX * scale)
    assert (got[~hit] == 0).all()


@pytest.mark.gpu
def test_square_light_behind_the_glass_sphere_matches_the_restatement(glass):
    """The refractive occluder of Phong.cpp:99-113 under samples = 4: rays whose shadow rays leave the sphere from inside are
    scaled by dot(N, l), the others skipped; against the restatement, the restatement's own fragile rays left out."""
    lights, samples = [LIGHT_A], 4
    uv = glass.uv(1, samples)
    want, blocked, fragile = glass.restate(lights, samples, uv)
    _, got, counted = glass.shade(lights, samples, uv=uv)
    on_sphere = glass.hits["prim"] == 3
    through = glass.through[(1, samples)]
    keep = ~fragile
    scale = float(want.max())
    print("%d rays on the sphere, %d samples lit through it, %d fragile rays, scale %.4g" % (on_sphere.sum(), through, fragile.sum(), scale))
    assert on_sphere.sum() > 0 and through > 0 and fragile.sum() <= 2
    assert counted == len(glass.idx) * samples
    assert np.allclose(got[keep], want[keep], rtol=RTOL, atol=ATOL_OF_MAX * scale)


@pytest.mark.gpu
def test_square_light_pixels_are_weight_times_L_over_spp(plain):
    """Every pixel receives one addition (d_pixels is a permutation, d_rgb zeroed): d_rgb[pixel] equals, as uint32,
    weight * L / spp of the ray's d_ray_rgb."""
    torch = plain.torch
    n, spp = plain.n, 2
    rng = np.random.RandomState(3)
    w = rng.rand(n, 3).astype(F)
    perm = rng.permutation(n).astype(np.int32)
    uv = plain.uv(2, 4)
    rgb, per_ray, _ = plain.shade([LIGHT_A, LIGHT_B], 4, uv=uv, weights=torch.from_numpy(w).cuda(), pixels=torch.from_numpy(perm).cuda(),
                                  spp=spp, n_pixels=n)
    want = np.zeros((n, 3), F)
    want[perm] = ((per_ray * w).astype(F) * (F(1.0) / F(spp))).astype(F)
    assert per_ray.max() > 0 and np.array_equal(rgb.view(np.uint32), want.view(np.uint32))
    assert np.array_equal(want[perm], ((per_ray * w).astype(F) / F(spp)).astype(F))            # halving is exact: the same as / spp


@pytest.mark.gpu
def test_square_light_internal_generator(plain):
    """d_uv_in NULL: the same seed gives the same bits and another seed others; at samples = 49 the floor's penumbra values lie
    between the umbra's and the lit region's (regions: the explicit-pair checker's classification of the same batch)."""
    _, a, counted = plain.shade([LIGHT_A], 49, seed=5)
    _, b, _ = plain.shade([LIGHT_A], 49, seed=5)
    _, c, _ = plain.shade([LIGHT_A], 49, seed=6)
    assert a.tobytes() == b.tobytes() and a.tobytes() != c.tobytes() and counted == len(plain.idx) * 49
    _, blocked, _ = plain.restate([LIGHT_A], 49, plain.uv(1, 49))
    floor = (plain.hits["prim"] == 0) | (plain.hits["prim"] == 1)
    v = a.sum(axis=1)
    umbra, lit = v[floor & (blocked[:, 0] == 49)], v[floor & (blocked[:, 0] == 0)]
    pen = v[floor & (blocked[:, 0] > 0) & (blocked[:, 0] < 49)]
    print("floor rays: %d umbra (mean %.4g), %d penumbra (mean %.4g), %d lit (mean %.4g)" % (len(umbra), umbra.mean(), len(pen), pen.mean(), len(lit), lit.mean()))
    assert len(umbra) and len(pen) and len(lit)
    assert umbra.min() <= pen.min() and pen.max() <= lit.max() and (pen >= 0).all()
    assert umbra.mean() < pen.mean() < lit.mean()


@pytest.mark.gpu
def test_square_light_refusals_on_the_device(plain, glass):
    """A non-square sample count is refused on a resident scene too; MR_TRACE_ANY is taken on opaque occluders (the same bits:
    any occluder scales the sample to 0) and refused with a refractive material."""
    from miro_amd import binding
    with pytest.raises(plain.miro.MiroError) as e:
        plain.shade([LIGHT_A], 8)
    assert e.value.status == binding.MR_ERR_INVALID
    uv = plain.uv(1, 4)
    _, closest, _ = plain.shade([LIGHT_A], 4, uv=uv)
    _, any_hit, _ = plain.shade([LIGHT_A], 4, uv=uv, flags=binding.MR_TRACE_ANY | binding.MR_MATH_PRODUCT)
    _, product, _ = plain.shade([LIGHT_A], 4, uv=uv, flags=binding.MR_MATH_PRODUCT)
    assert np.array_equal(any_hit.view(np.uint32), product.view(np.uint32)) and np.array_equal(product.view(np.uint32), closest.view(np.uint32))
    with pytest.raises(glass.miro.MiroError) as e:
        glass.shade([LIGHT_A], 4, flags=binding.MR_TRACE_ANY)
    assert e.value.status == binding.MR_ERR_STATE


@pytest.mark.gpu
def test_frame_renderer_opt_in_paths(miro):
    """FrameRenderer(lens=...) generates the lens call's rays; square_lights= adds mr_shade_square_lights' light to every level
    of the batched path; without the options the frame is the same bits as before."""
    import torch
    from miro_amd import frame, scenes
    desc = scenes.SCENES["teapot"]
    s = miro.Scene(0)
    scenes.populate(s, desc)
    s.build(4)
    W = H = 24
    base = frame.FrameRenderer(s, desc, W, H, spp=2)
    base.generate()
    base.render_specular(depth=0)
    lensed = frame.FrameRenderer(s, desc, W, H, spp=2, lens=dict(aperture=0.2, focus_plane=6.7))
    lensed.generate()
    want = torch.empty_like(lensed.d_rays)
    s.gen_eye_rays_lens(lensed.cam, W, H, want, 0.2, 6.7, spp=2, jitter=True, seed=168)
    torch.cuda.synchronize()
    assert torch.equal(lensed.d_rays, want) and not torch.equal(lensed.d_rays, base.d_rays)
    with pytest.raises(ValueError):
        frame.FrameRenderer(s, desc, W, H, spp=2, lens=dict(aperture=0.2, focus_plane=6.7), tiled=True)
    sq = dict(position=(0.0, 8.0, 0.0), normal=(0.0, -1.0, 0.0), wattage=300.0, dimensions=(2.0, 2.0))
    both = frame.FrameRenderer(s, desc, W, H, spp=2, square_lights=[sq], square_samples=4)
    both.generate()
    levels = both.render_specular(depth=0)
    torch.cuda.synchronize()
    only = torch.zeros_like(both.d_rgb)
    s.shade_square_lights([sq], 4, both.d_rays, base_hits(s, both), both.n, only, seed=168, spp=2)
    torch.cuda.synchronize()
    assert torch.equal(both.d_rays, base.d_rays) and float(only.max()) > 0
    assert torch.allclose(both.d_rgb, base.d_rgb + only, rtol=1e-5, atol=1e-7 * float(both.d_rgb.max()))
    assert levels[0][1] == 5 * base.render_specular(depth=0)[0][1]                              # 1 point + 4 square shadow rays per hit
    with pytest.raises(ValueError):
        both.render_specular(depth=0, fused=True)


def base_hits(scene, fr):
    import torch
    hits = torch.empty((fr.n, 4), dtype=torch.float32, device="cuda")
    scene.trace_device(fr.d_rays, fr.n, hits)
    return hits
