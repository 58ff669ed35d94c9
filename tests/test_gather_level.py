"""mr_gather_level -- the photon-map term of Scene::traceScene (Scene.cpp:286-299) for any queue of the recursion -- and
FrameRenderer.render_specular(photon_maps=...), which calls it at every level.

Every expectation comes from ORACLE maps: the records the product's photon walk traced (held by tests/test_photon_walk.py and
tests/test_photon_walk_surface.py) go through the oracle's store, scale_photon_power(1 / emitted) and balance, the product's
balanced map must equal that map (same_map), and the queries go to oracle.PhotonMap.irradiance_estimate at the device's own
mr_hit_attrs P and at the normal the call was given.  Which rays are queries is decided on the host from the hit records and
the material table.  The code under test is never its own yardstick.

Queries at which two photons inside the search radius lie at exactly the same fp32 squared distance are left out of the value
comparisons (tied_queries of test_photon_walk.py: such a tie can change which photon the k-th nearest is); the census test
below holds them to 1 % of every level with the oracle alone."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import kernel_budget  # noqa: E402
from test_photon_walk import (K_GATHER, MAX_DIST, MISS, PLANE_BIT, W_GATHER, gather_setup, material_table, oracle_map, oracle_room,  # noqa: E402
                              product_room, product_trace, same_map, tied_queries)

F = np.float32
RTOL = 2e-5           # of the largest expected value: test_traced_maps_answer_queries_like_the_oracles' tolerance for traced maps
TARGETS = ((False, 6000), (True, 2500))


def normalised(N):
    """Vector3::normalize as Scene.cpp:262 applies it: *= 1 / length, every operation a float32 one"""
    N = np.ascontiguousarray(N, F)
    with np.errstate(divide="ignore", invalid="ignore"):
        return (N * (F(1) / np.sqrt((N[:, 0] * N[:, 0] + N[:, 1] * N[:, 1]) + N[:, 2] * N[:, 2]))[:, None]).astype(F)


def diffuse_hits(desc, prim):
    """Phong::isDiffuse (Phong.cpp:39-42) of every hit record's material, from the description's tables: a plane carries its
    material id, a bounded object looks it up; a miss is no hit"""
    prim = np.asarray(prim, np.uint32)
    kd = material_table(desc)[:, 0:3]
    plane_mat = np.array([o[3] if len(o) > 3 else 0 for o in desc["objects"] if o[0] == "plane"] + [0], np.uint32)
    prim_mat = np.asarray(desc["prim_material"], np.uint32)
    hit = prim != np.uint32(MISS)
    is_plane = hit & ((prim & np.uint32(PLANE_BIT)) != 0)
    mid = np.where(is_plane, plane_mat[np.where(is_plane, prim & np.uint32(0x7FFFFFFF), 0)], prim_mat[np.where(hit & ~is_plane, prim, 0)])
    return hit & (kd[mid] > 0).any(axis=1)


# ---- without a GPU -------------------------------------------------------------------------------------------------------
def test_symbols_and_argument_errors(miro):
    """The library exports mr_gather_level, SURFACE_SYMBOLS lists it, miro_hip_surface.h declares it and miro_hip.h's own list
    stays at 69 names.  The MR_ERR_INVALID cases answer before any device call, in the documented order (this runs on a machine
    without a device): a later error never hides an earlier one."""
    from miro_amd import binding
    L = miro.lib()
    assert hasattr(L, "mr_gather_level") and "mr_gather_level" in binding.SURFACE_SYMBOLS
    assert "mr_gather_level" not in binding.EXPORTED_SYMBOLS and len(binding.EXPORTED_SYMBOLS) == 69
    strip = lambda p: re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", p)).read(), flags=re.S)
    assert re.search(r"\bmr_status\s+mr_gather_level\s*\(", strip("miro_hip_surface.h"))
    assert not re.search(r"\bmr_gather_level\s*\(", strip("miro_hip.h"))
    assert "mr_gather_level" in open(os.path.join(ROOT, "include", "miro_hip.h")).read()          # the doc comment

    host = miro.Scene()
    host.add_triangle([0, 0, 0, 1, 0, 0, 0, 1, 0], [0, 0, 1] * 3)
    host.build(4, host_only=True)
    unbuilt = miro.Scene()
    unbuilt.add_triangle([0, 0, 0, 1, 0, 0, 0, 1, 0], [0, 0, 1] * 3)
    m = miro.PhotonMap(100)                                     # not balanced
    elsewhere = miro.PhotonMap(100, device=1)
    A = 4096                                                    # an aligned, non-NULL address that is never dereferenced

    def call(scene=host.h, g=None, c=None, rays=A, hits=A, normal=None, weights=None, pixels=None, n=64, max_dist=1.0, k=50, spp=1,
             scratch=A, rgb=A, ray_rgb=None, counts=None):
        return L.mr_gather_level(scene, g, c, rays, hits, normal, weights, pixels, n, max_dist, k, spp, scratch, rgb, ray_rgb, counts, None)

    for kw in (dict(scene=None), dict(rays=None), dict(hits=None), dict(scratch=None), dict(rgb=None, ray_rgb=None)):
        assert call(spp=0, k=0, **kw) == -1 and b"NULL" in L.mr_last_error(), kw
    assert call(spp=0, k=0) == -1 and b"spp" in L.mr_last_error()
    for k in (0, 513):
        assert call(k=k, rays=A + 4) == -1 and b"nphotons" in L.mr_last_error()
    for kw in (dict(rays=A + 4), dict(hits=A + 8), dict(counts=A + 4), dict(rgb=A + 2), dict(ray_rgb=A + 1), dict(weights=A + 2),
               dict(pixels=A + 2), dict(normal=A + 3), dict(scratch=A + 2)):
        assert call(g=elsewhere.h, **kw) == -1 and b"aligned" in L.mr_last_error(), kw
    assert call(g=elsewhere.h, scene=unbuilt.h) == -1 and b"device" in L.mr_last_error()
    assert call(c=elsewhere.h) == -1 and b"device" in L.mr_last_error()
    assert call(scene=unbuilt.h, g=m.h) == -5 and b"mr_bvh_build" in L.mr_last_error()
    assert call(g=m.h) == -5 and b"CPU" in L.mr_last_error()                      # host_only: never a CPU gather
    assert call(g=m.h, n=0) == -5
    assert call(rgb=None, ray_rgb=A) == -5                                        # one output suffices: the next check answers


def test_gather_level_kernels_stay_inside_the_verified_envelope():
    """Both kernels of mr_gather_level.hip: no scratch, no spills, no dynamic stack, and no fewer waves per SIMD than their own
    record (tests/golden/kernel_budget_gather_level.json, written from the build whose GPU run of this file was green) and than
    the worst kernel of tests/golden/kernel_budget.json."""
    cur = kernel_budget.unit_kernels("mr_gather_level")
    assert len(cur) == 2 and any("gather_level_queries_kernel" in k for k in cur) and any("gather_level_accumulate_kernel" in k for k in cur)
    for name, c in cur.items():
        assert c["scratch_bytes_per_lane"] == 0 and c["vgprs_spilled"] == 0 and c["sgprs_spilled"] == 0, (name, c)
    kernel_budget.assert_inside_envelope(cur, "kernel_budget_gather_level.json")


def test_tie_census_with_the_oracle_alone(oracle):
    """What keeps the value comparisons honest: the 48 x 48 photon_room frame and its children down three levels (the oracle's
    path_rays(kinds=3), level by level; the room's shininess is infinite, so the lobe-sampled children are the mirror and the
    refracted directions), against the restated maps of test_photon_walk.py.  At most 1 % of the hit points of any level have
    two photons at exactly the same fp32 squared distance inside MAX_DIST, for either map."""
    from helpers import camera_of
    maps, _, _ = gather_setup(oracle)
    s, desc = oracle_room(oracle, "photon_room")
    mats = material_table(desc)
    rays = oracle.eye_rays(camera_of(oracle, "photon_room"), W_GATHER, W_GATHER)
    weights = pixels = None
    sizes = []
    for level in range(4):
        hits = s.trace(rays)
        hit = hits["prim"] != MISS
        P, _ = s.hit_attrs(hits, rays)
        sizes.append(len(rays))
        for caustic in (False, True):
            tied = tied_queries(maps[caustic]["records"]["pos"], P[hit], MAX_DIST)
            print("level %d caustic=%d: %d of %d hit points tied" % (level, caustic, tied.sum(), hit.sum()))
            assert tied.sum() <= 0.01 * len(rays)
        if level == 3:
            break
        rays, weights, pixels, _, _ = s.path_rays(mats, desc["prim_material"], rays, hits, weights, pixels, spp=1, bounce=level, kinds=3)
    assert sizes[0] == W_GATHER * W_GATHER and all(n > 0 for n in sizes) and sizes[1] % 64 != 0


# ---- on the MI355X -------------------------------------------------------------------------------------------------------
def camera(miro, desc):
    return miro.binding.make_camera(desc["eye"], desc["lookat"], desc["up"], desc["fov"])


def traced_maps(oracle, miro, scene, desc, targets=TARGETS, light=None, max_emissions=400000, **kw):
    """Per (caustic, target): the product's map, traced and balanced on the device; the oracle's map of the same records, which
    the product's map equals; the photon positions (for tied_queries)"""
    out = []
    for caustic, target in targets:
        m, res, recs = product_trace(miro, scene, desc, target, max_emissions, caustic, target + 64, target + 64, light=light, **kw)
        assert target <= res["stored"] <= target + 64
        m.balance()
        ref = oracle_map(oracle, dict(records=recs, emitted=res["emitted"]), target + 64)
        same_map(m, ref)
        out.append((m, ref, recs["pos"].copy()))
    return out


class Level:
    """One queue of the recursion, traced: device rays / hits / weights / pixels, and on the host which rays are queries, the
    device's mr_hit_attrs P and the normalised N of the object"""

    def __init__(self, miro, scene, desc, rays, weights, pixels, n, flags=0):
        import torch
        self.n, self.rays, self.weights, self.pixels = n, rays, weights, pixels
        self.hits = torch.empty((n, 4), dtype=torch.float32, device="cuda")
        scene.trace_device(rays, n, self.hits, flags)
        dP, dN = (torch.zeros((n, 3), dtype=torch.float32, device="cuda") for _ in range(2))
        scene.hit_attrs(self.hits, n, dP, dN, d_rays=rays)
        torch.cuda.synchronize()
        self.prim = self.hits.cpu().numpy().view(miro.HIT_DTYPE).reshape(-1)["prim"].copy()
        self.hit = self.prim != MISS
        self.query = diffuse_hits(desc, self.prim)
        self.P, self.N = dP.cpu().numpy(), normalised(dN.cpu().numpy())
        self.w = weights.cpu().numpy().astype(np.float64) if weights is not None else np.ones((n, 3))

    def pixel_index(self, spp):
        return self.pixels.cpu().numpy().astype(np.int64) if self.pixels is not None else np.arange(self.n) // spp


def make_levels(miro, scene, desc, W, H, spp=1, depth=0):
    """trace_device -> gen_secondary_rays by hand, as render_specular's batched path queues them"""
    import torch
    n = W * H * spp
    rays = torch.empty((n, 8), dtype=torch.float32, device="cuda")
    scene.gen_eye_rays(camera(miro, desc), W, H, rays, spp=spp, jitter=spp > 1)
    weights = pixels = None
    out = []
    for level in range(depth + 1):
        out.append(Level(miro, scene, desc, rays, weights, pixels, n, miro.MR_TRACE_INCOHERENT if level else 0))
        if level == depth:
            break
        o_rays = torch.empty((3 * n, 8), dtype=torch.float32, device="cuda")
        o_w = torch.empty((3 * n, 3), dtype=torch.float32, device="cuda")
        o_pix = torch.empty(3 * n, dtype=torch.int32, device="cuda")
        cnt = torch.zeros(1, dtype=torch.int64, device="cuda")
        scene.gen_secondary_rays(rays, out[-1].hits, weights, pixels, n, o_rays, o_w, o_pix, cnt, spp=spp)
        n = int(cnt.item())
        rays, weights, pixels = o_rays[:n].contiguous(), o_w[:n].contiguous(), o_pix[:n].contiguous()
    return out


def expect(maps, lv, N=None, max_dist=MAX_DIST, k=K_GATHER):
    """The oracle's estimates at the level's queries (0 elsewhere), per map, and per map the queries with an exact distance tie"""
    N = lv.N if N is None else N
    q = np.nonzero(lv.query)[0]
    E, tied = [], []
    for m, ref, pos in maps:
        e, t = np.zeros((lv.n, 3), F), np.zeros(lv.n, bool)
        if len(q):
            e[q] = ref.irradiance_estimate(lv.P[q], N[q], max_dist=max_dist, nphotons=k)[0]
            t[q] = tied_queries(pos, lv.P[q], max_dist)
        assert lv.n < 1000 or t.sum() <= 0.01 * lv.n             # the census test's cap (a frame of 25 rays has no such share)
        E.append(e)
        tied.append(t)
    return E, tied


def gather(scene, g, c, lv, normal=None, rgb=None, spp=1, weights="level", pixels="level", max_dist=MAX_DIST, k=K_GATHER, want_rays=True):
    """One mr_gather_level over a level; returns (d_ray_rgb, scratch [4, n, 3], counts) on the host"""
    import torch
    scratch = torch.full((12 * lv.n,), -3.0, dtype=torch.float32, device="cuda")
    ray_rgb = torch.full((lv.n, 3), -3.0, dtype=torch.float32, device="cuda") if want_rays else None
    counts = torch.zeros(2, dtype=torch.int64, device="cuda")
    scene.gather_level(g, c, lv.rays, lv.hits, lv.n, scratch, rgb, d_normal=normal, d_weights=lv.weights if weights == "level" else weights,
                       d_pixels=lv.pixels if pixels == "level" else pixels, max_dist=max_dist, nphotons=k, spp=spp, d_ray_rgb=ray_rgb,
                       d_counts=counts)
    torch.cuda.synchronize()
    return (ray_rgb.cpu().numpy() if want_rays else None), scratch.cpu().numpy().reshape(4, lv.n, 3), counts.tolist()


def close_on(got, want, keep, what):
    scale = float(np.abs(want[keep]).max())
    err = float(np.abs(got[keep].astype(np.float64) - want[keep]).max())
    print("%s: %d values compared, largest expected %.4g, worst error %.3g (bound %.3g)" % (what, keep.sum(), scale, err, RTOL * scale))
    assert scale > 0 and err <= RTOL * scale


_ROOM = {}


def room(oracle, miro):
    """photon_room with its two maps and the three levels of the 48 x 48 frame at one sample per pixel, made once"""
    if not _ROOM:
        scene, desc = product_room(miro, "photon_room")
        maps = traced_maps(oracle, miro, scene, desc)
        levels = make_levels(miro, scene, desc, W_GATHER, W_GATHER, depth=2)
        _ROOM.update(scene=scene, desc=desc, maps=maps, levels=levels, expect=[expect(maps, lv) for lv in levels])
    return _ROOM


@pytest.mark.gpu
def test_queries(oracle, miro):
    """The level-1 queue of the 48 x 48 frame (no multiple of 64 rays; it has weights and pixels): the positions in d_scratch are
    mr_hit_attrs' P and the normals the normalised N, bit for bit, on the rays whose hit is diffuse; the normal is NaN exactly on
    the others; d_counts is (diffuse hits counted on the host, rays), added to what it held."""
    import torch
    r = room(oracle, miro)
    lv = r["levels"][1]
    g, c = r["maps"][0][0], r["maps"][1][0]
    _, scratch, counts = gather(r["scene"], g, c, lv)
    q = lv.query
    print("level 1: %d rays, %d queries" % (lv.n, q.sum()))
    assert lv.n % 64 != 0 and lv.weights is not None and lv.pixels is not None
    assert 0 < q.sum() < lv.n and counts == [int(q.sum()), lv.n]
    assert np.array_equal(scratch[0][q].view(np.uint32), lv.P[q].view(np.uint32))
    assert np.array_equal(scratch[1][q].view(np.uint32), lv.N[q].view(np.uint32))
    assert np.array_equal(np.isnan(scratch[1]).all(axis=1), ~q) and np.array_equal(np.isnan(scratch[1]).any(axis=1), ~q)
    assert (scratch[2][~q] == 0).all() and (scratch[3][~q] == 0).all()
    # d_counts is added to, not zeroed
    cnt = torch.tensor([5, 7], dtype=torch.int64, device="cuda")
    out = torch.empty((lv.n, 3), dtype=torch.float32, device="cuda")
    r["scene"].gather_level(g, None, lv.rays, lv.hits, lv.n, torch.empty(12 * lv.n, dtype=torch.float32, device="cuda"), None,
                            max_dist=MAX_DIST, nphotons=K_GATHER, d_ray_rgb=out, d_counts=cnt)
    torch.cuda.synchronize()
    assert cnt.tolist() == [5 + int(q.sum()), 7 + lv.n]


@pytest.mark.gpu
def test_per_ray_term(oracle, miro):
    """The same queue with both maps, then each alone: d_ray_rgb is the oracle's irradiance + caustic (one float add), or the one
    map's estimate, within 2e-5 of the largest expected value on the queries without a tie, and 0 on every ray that is no query."""
    r = room(oracle, miro)
    lv, (E, tied) = r["levels"][1], r["expect"][1]
    g, c = r["maps"][0][0], r["maps"][1][0]
    for name, mg, mc, want, t in (("both maps", g, c, E[0] + E[1], tied[0] | tied[1]), ("global alone", g, None, E[0], tied[0]),
                                  ("caustic alone", None, c, E[1], tied[1])):
        got, scratch, _ = gather(r["scene"], mg, mc, lv)
        assert (got[~lv.query] == 0).all()
        close_on(got, want.astype(np.float64), lv.query & ~t, name)
        if mg is not None and mc is not None:                   # the two estimates stay in the scratch, where the contract puts them
            assert np.array_equal((scratch[2] + scratch[3]).view(np.uint32), got.view(np.uint32))


@pytest.mark.gpu
def test_the_normal_buffer_is_what_the_facing_test_reads(oracle, miro):
    """d_normal = the geometric normals, negated on every second ray: the result is the oracle's at THOSE normals -- which differs
    from the oracle's at the un-flipped normals on some flipped ray, so a call that ignored the buffer would fail.  With the
    un-flipped normals in the buffer, d_ray_rgb is the d_normal = NULL run's bit for bit."""
    import torch
    r = room(oracle, miro)
    lv, (E, tied) = r["levels"][1], r["expect"][1]
    g, c = r["maps"][0][0], r["maps"][1][0]
    flipped = (np.arange(lv.n) % 2) == 1
    N = np.where(lv.hit[:, None], lv.N, F(0)).astype(F)
    Nf = np.where(flipped[:, None], -N, N).astype(F)
    Ef, tf = expect(r["maps"], lv, N=Nf)
    keep = lv.query & ~(tf[0] | tf[1])
    plain = (E[0] + E[1]).astype(np.float64)
    want = (Ef[0] + Ef[1]).astype(np.float64)
    differs = (np.abs(want - plain).max(axis=1) > 10 * RTOL * np.abs(plain).max()) & keep & flipped
    print("%d of %d flipped queries change their estimate" % (differs.sum(), (keep & flipped).sum()))
    assert differs.any()
    got, scratch, _ = gather(r["scene"], g, c, lv, normal=torch.from_numpy(Nf).cuda())
    assert np.array_equal(scratch[1][lv.query].view(np.uint32), Nf[lv.query].view(np.uint32))
    assert np.isnan(scratch[1][~lv.query]).all() and (got[~lv.query] == 0).all()
    close_on(got, want, keep, "flipped normals")
    same, _, _ = gather(r["scene"], g, c, lv, normal=torch.from_numpy(N).cuda())
    null, _, _ = gather(r["scene"], g, c, lv)
    assert same.tobytes() == null.tobytes()


def pixel_sums(lv, E, tied, spp, n_pixels):
    """sum of weight * E / spp over every pixel's rays in float64, and the pixels that receive a tied query"""
    px = lv.pixel_index(spp)
    want = np.zeros((n_pixels, 3), np.float64)
    np.add.at(want, px, lv.w * (E[0] + E[1]).astype(np.float64) / spp)
    bad = np.zeros(n_pixels, bool)
    bad[px[tied[0] | tied[1]]] = True
    return want, bad


def check_pixels(added, before_max, want, bad, what):
    """2e-5 of the largest expected pixel + 4e-7 of the largest pixel before the call (the rounding of a difference of two fp32
    pictures, as in tests/test_photon.py::test_final_gather_frame_matches_oracle)"""
    bound = RTOL * float(want.max()) + 4e-7 * before_max
    err = float(np.abs(added - want)[~bad].max())
    print("%s: largest expected pixel %.4g, %d pixels with a tie left out, worst error %.3g (bound %.3g)" % (what, want.max(), bad.sum(), err, bound))
    assert want.max() > 0 and err <= bound


@pytest.mark.gpu
def test_weighted_pixel_sums(oracle, miro):
    """Levels 0, 1 and 2 by hand (trace_device -> gather_level -> gen_secondary_rays) at one sample per pixel, level 0 at two
    samples with pixels = NULL (the k / spp path, runs of two equal pixels), and a 5 x 5 frame (25 rays: less than a wave): what
    the call ADDS to a d_rgb that already holds a picture is the float64 sum of weight * E / spp over the pixel's rays, E the
    oracle's."""
    import torch
    r = room(oracle, miro)
    scene, desc, maps = r["scene"], r["desc"], r["maps"]
    g, c = maps[0][0], maps[1][0]
    cases = [("level %d" % i, lv, ex, 1, W_GATHER * W_GATHER) for i, (lv, ex) in enumerate(zip(r["levels"], r["expect"]))]
    two = make_levels(miro, scene, desc, W_GATHER, W_GATHER, spp=2)[0]
    small = make_levels(miro, scene, desc, 5, 5)[0]
    cases += [("level 0 at 2 spp", two, expect(maps, two), 2, W_GATHER * W_GATHER), ("5 x 5", small, expect(maps, small), 1, 25)]
    assert two.pixels is None and two.n == 2 * W_GATHER * W_GATHER and small.n == 25
    rng = np.random.RandomState(5)
    for what, lv, (E, tied), spp, n_pixels in cases:
        before = rng.rand(n_pixels, 3).astype(F)
        rgb = torch.from_numpy(before).cuda()
        gather(scene, g, c, lv, rgb=rgb, spp=spp, want_rays=False)
        want, bad = pixel_sums(lv, E, tied, spp, n_pixels)
        check_pixels(rgb.cpu().numpy().astype(np.float64) - before.astype(np.float64), float(before.max()), want, bad, what)


@pytest.mark.gpu
def test_the_driver_gathers_at_every_level(oracle, miro):
    """render_specular(depth=2, photon_maps=(g, c)) minus the same frame without maps is the sum of the three levels' terms, restated
    as in test_weighted_pixel_sums; the rays per level are the same in both runs; levels 1 and 2 alone light some pixel (a driver
    that gathered at level 0 only would miss that part); fused=True with photon_maps raises ValueError."""
    import torch
    from miro_amd import frame
    r = room(oracle, miro)
    g, c = r["maps"][0][0], r["maps"][1][0]
    fr = frame.FrameRenderer(r["scene"], r["desc"], W_GATHER, W_GATHER)
    fr.generate()
    levels0 = fr.render_specular(depth=2)
    torch.cuda.synchronize()
    plain = fr.d_rgb.cpu().numpy().astype(np.float64)
    levels1 = fr.render_specular(depth=2, photon_maps=(g, c), nphotons=K_GATHER, max_dist=MAX_DIST)
    torch.cuda.synchronize()
    lit = fr.d_rgb.cpu().numpy().astype(np.float64)
    assert levels0 == levels1 and [n for n, _ in levels1] == [lv.n for lv in r["levels"]]
    n_pixels = W_GATHER * W_GATHER
    want, bad, deeper = np.zeros((n_pixels, 3)), np.zeros(n_pixels, bool), np.zeros((n_pixels, 3))
    for i, (lv, (E, tied)) in enumerate(zip(r["levels"], r["expect"])):
        w, b = pixel_sums(lv, E, tied, 1, n_pixels)
        want += w
        bad |= b
        if i:
            deeper += w
    print("levels 1-2 add at most %.4g to a pixel, all levels %.4g" % (deeper.max(), want.max()))
    assert deeper.max() > 0
    check_pixels(lit - plain, float(plain.max()), want, bad, "depth-2 frame")
    seen_deeper = (deeper.max(axis=1) > 100 * (RTOL * want.max() + 4e-7 * plain.max())) & ~bad
    assert seen_deeper.any()
    with pytest.raises(ValueError):
        fr.render_specular(depth=2, fused=True, photon_maps=(g, c))
    with pytest.raises(ValueError):
        fr.render_specular(depth=2, fused="auto", photon_maps=(g, None))


@pytest.mark.gpu
def test_stone_scene(oracle, miro):
    """scenes.photon_room_stone() with maps from trace_photons(surface=True): without a normal buffer the call is refused
    (MR_ERR_STATE, naming mr_hit_surface); with mr_hit_surface's buffer the per-ray term is the oracle's at that buffer's normals
    -- which are not the geometric ones on the stone; and render_specular(photon_maps=...) at depth 0 and one sample per pixel is
    the same sequence of calls made by hand, byte for byte."""
    import torch
    from miro_amd import frame, scenes
    desc = scenes.photon_room_stone()
    scene = miro.Scene(0)
    scenes.textured_room_setup(scene, desc)
    maps = traced_maps(oracle, miro, scene, desc, surface=True)
    g, c = maps[0][0], maps[1][0]
    lv = make_levels(miro, scene, desc, W_GATHER, W_GATHER)[0]
    with pytest.raises(miro.MiroError) as e:
        gather(scene, g, c, lv)
    assert e.value.status == -5 and "mr_hit_surface" in str(e.value)
    color, normal = (torch.zeros((lv.n, 3), dtype=torch.float32, device="cuda") for _ in range(2))
    scene.hit_surface(lv.rays, lv.hits, lv.n, color, normal)
    torch.cuda.synchronize()
    Nb = normal.cpu().numpy()
    bent = (Nb.view(np.uint32) != lv.N.view(np.uint32)).any(axis=1) & lv.query
    print("%d of %d queries have a bumped normal" % (bent.sum(), lv.query.sum()))
    assert bent.sum() > 100
    E, tied = expect(maps, lv, N=Nb)
    got, scratch, _ = gather(scene, g, c, lv, normal=normal)
    assert np.array_equal(scratch[1][lv.query].view(np.uint32), Nb[lv.query].view(np.uint32)) and (got[~lv.query] == 0).all()
    close_on(got, (E[0] + E[1]).astype(np.float64), lv.query & ~(tied[0] | tied[1]), "bumped normals")
    # the driver
    fr = frame.FrameRenderer(scene, desc, W_GATHER, W_GATHER)
    fr.generate()
    fr.render_specular(depth=0, lights=desc["lights"], photon_maps=(g, c), nphotons=K_GATHER, max_dist=MAX_DIST)
    torch.cuda.synchronize()
    driver = fr.d_rgb.cpu().numpy().copy()
    hand = torch.zeros((fr.n, 3), dtype=torch.float32, device="cuda")
    hits = torch.empty((fr.n, 4), dtype=torch.float32, device="cuda")
    scene.trace_device(fr.d_rays, fr.n, hits)
    scene.hit_surface(fr.d_rays, hits, fr.n, color, normal)
    scene.shade_lights_surface(fr.d_rays, hits, color, normal, fr.n, hand)
    scene.gather_level(g, c, fr.d_rays, hits, fr.n, torch.empty(12 * fr.n, dtype=torch.float32, device="cuda"), hand, d_normal=normal,
                       max_dist=MAX_DIST, nphotons=K_GATHER)
    torch.cuda.synchronize()
    assert driver.tobytes() == hand.cpu().numpy().tobytes() and driver.max() > 0


@pytest.mark.gpu
def test_the_references_final_scene(oracle, miro):
    """scenes.flower_scene() with a global map of about 4000 photons from its disc light (the surface walk), 48 x 32, its light
    list and its background: render_specular(photon_maps=(g, None), nphotons=50) is trace -> shade_environment -> hit_surface ->
    shade_lights_surface -> gather_level made by hand, byte for byte (no material has ks or kt: one level), and the photon term
    lights some petal pixel."""
    import torch
    from miro_amd import frame, scenes
    scene = miro.Scene(0)
    desc = scenes.flower_setup(scene)
    (g, ref, pos), = traced_maps(oracle, miro, scene, desc, targets=((False, 4000),), light=desc["lights"][0], max_emissions=4000000, surface=True)
    W, H = 48, 32
    fr = frame.FrameRenderer(scene, desc, W, H)
    fr.generate()
    levels = fr.render_specular(depth=3, lights=desc["lights"], environment=True, photon_maps=(g, None), nphotons=50)
    torch.cuda.synchronize()
    driver = fr.d_rgb.cpu().numpy().copy()
    assert len(levels) == 1
    n = fr.n
    hand, color, normal, term = (torch.zeros((n, 3), dtype=torch.float32, device="cuda") for _ in range(4))
    hits = torch.empty((n, 4), dtype=torch.float32, device="cuda")
    scene.trace_device(fr.d_rays, n, hits)
    scene.shade_environment(fr.d_rays, hits, n, hand)
    scene.hit_surface(fr.d_rays, hits, n, color, normal)
    scene.shade_lights_surface(fr.d_rays, hits, color, normal, n, hand)
    scene.gather_level(g, None, fr.d_rays, hits, n, torch.empty(12 * n, dtype=torch.float32, device="cuda"), hand, d_normal=normal,
                       nphotons=50, d_ray_rgb=term)
    torch.cuda.synchronize()
    assert driver.tobytes() == hand.cpu().numpy().tobytes()
    prim = hits.cpu().numpy().view(miro.HIT_DTYPE).reshape(-1)["prim"]
    petal = prim < 14784                                        # the triangles of Petals2.obj come first
    t = term.cpu().numpy()
    print("%d petal pixels, photon term up to %.4g on them" % (petal.sum(), t[petal].max()))
    assert petal.any() and t[petal].max() > 0 and (t[prim == MISS] == 0).all()


@pytest.mark.gpu
def test_plain_equivalence_with_final_gather(oracle, miro):
    """A level-0 batch with weights = pixels = d_normal = NULL at one sample per pixel: what the call adds to a zeroed frame agrees
    with mr_final_gather's on a second zeroed frame within 1e-6 of the largest value (both add one float to the pixel).  n = 0 is
    MR_OK; with both maps NULL the call is valid and adds nothing."""
    import torch
    r = room(oracle, miro)
    scene, lv = r["scene"], r["levels"][0]
    g, c = r["maps"][0][0], r["maps"][1][0]
    a, b = (torch.zeros((lv.n, 3), dtype=torch.float32, device="cuda") for _ in range(2))
    scratch = torch.empty(12 * lv.n, dtype=torch.float32, device="cuda")
    scene.gather_level(g, c, lv.rays, lv.hits, lv.n, scratch, a, max_dist=MAX_DIST, nphotons=K_GATHER)
    scene.final_gather(g, c, lv.rays, lv.hits, lv.n, scratch, b, max_dist=MAX_DIST, nphotons=K_GATHER)
    torch.cuda.synchronize()
    a_h, b_h = a.cpu().numpy(), b.cpu().numpy()
    print("largest pixel %.4g, largest difference %.3g" % (b_h.max(), np.abs(a_h - b_h).max()))
    assert b_h.max() > 0 and np.abs(a_h - b_h).max() <= 1e-6 * b_h.max()
    scene.gather_level(g, c, lv.rays, lv.hits, 0, scratch, a, max_dist=MAX_DIST, nphotons=K_GATHER)
    scene.gather_level(None, None, lv.rays, lv.hits, lv.n, scratch, a, max_dist=MAX_DIST, nphotons=K_GATHER)
    torch.cuda.synchronize()
    assert a.cpu().numpy().tobytes() == a_h.tobytes()


# a triangle mesh (a diffuse quad, a glass triangle in front of it), a diffuse and a mirror sphere, a diffuse floor plane, open sky
QUERY_SCENE = dict(
    models=[], floor=None,
    objects=[("tri", (-0.5, 0.0, 0.0, 0.5, 0.0, 0.0, 0.5, 1.0, 0.0), (0.0, 0.0, 1.0) * 3),
             ("tri", (-0.5, 0.0, 0.0, 0.5, 1.0, 0.0, -0.5, 1.0, 0.0), (0.0, 0.0, 1.0) * 3),
             ("tri", (-0.4, 0.0, 1.5, 0.4, 0.0, 1.5, 0.0, 0.6, 1.5), (0.0, 0.0, 1.0) * 3),
             ("sphere", (-1.4, 0.6, 0.0), 0.6), ("sphere", (1.4, 0.6, 0.0), 0.6),
             ("plane", (0.0, 1.0, 0.0), (0.0, 0.0, 0.0), 0)],
    materials=[((0.7, 0.6, 0.5), (0.0, 0.0, 0.0), (0.0, 0.0, 0.0), float("inf"), 1.0),
               ((0.0, 0.0, 0.0), (0.9, 0.9, 0.9), (0.0, 0.0, 0.0), float("inf"), 1.0),
               ((0.0, 0.0, 0.0), (0.05, 0.05, 0.05), (0.9, 0.9, 0.9), float("inf"), 1.5)],
    prim_material=[0, 0, 2, 0, 1],
    eye=(0.0, 1.5, 6.0), lookat=(0.0, 0.5, 0.0), up=(0.0, 1.0, 0.0), fov=45.0)


def query_kinds(desc, prim):
    """per hit record: is it a query, and on which kind of object (0 triangle, 1 sphere, 2 plane; -1 miss)"""
    prim = np.asarray(prim, np.uint32)
    bounded = [o[0] for o in desc["objects"] if o[0] != "plane"]
    is_sphere = np.array([k == "sphere" for k in bounded] + [False])
    hit = prim != np.uint32(MISS)
    plane = hit & ((prim & np.uint32(PLANE_BIT)) != 0)
    kind = np.where(plane, 2, np.where(is_sphere[np.where(hit & ~plane, prim, len(bounded))], 1, 0))
    return diffuse_hits(desc, prim), np.where(hit, kind, -1)


@pytest.mark.gpu
def test_final_gather_and_gather_level_build_the_same_queries(miro):
    """mr_final_gather builds its queries with the kernel of mr_gather_level (d_normal = NULL): on one traced batch of 24 x 17 = 408
    rays (one full workgroup, one partial one, the last wave partial) at one sample per pixel, the first 6 n floats of the scratch --
    positions, then normals with NaN = no query -- are byte-equal after mr_final_gather and after mr_gather_level(d_normal =
    d_weights = d_pixels = NULL).  The batch holds a query on a triangle, on a sphere and on a plane, a hit that is no query (mirror,
    glass) and a miss."""
    import torch
    from miro_amd import scenes
    desc, W, H = QUERY_SCENE, 24, 17
    n = W * H
    scene = miro.Scene(0)
    scenes.populate(scene, desc)
    scene.set_materials(desc["materials"], desc["prim_material"])
    scene.build(4)
    rays = torch.empty((n, 8), dtype=torch.float32, device="cuda")
    hits = torch.empty((n, 4), dtype=torch.float32, device="cuda")
    scene.gen_eye_rays(camera(miro, desc), W, H, rays)
    scene.trace_device(rays, n, hits)
    torch.cuda.synchronize()
    prim = hits.cpu().numpy().view(miro.HIT_DTYPE).reshape(-1)["prim"]
    query, kind = query_kinds(desc, prim)
    print("%d rays: queries on triangles / spheres / planes %s, %d hits that are no query, %d misses"
          % (n, [int((query & (kind == k)).sum()) for k in range(3)], (~query & (kind >= 0)).sum(), (kind < 0).sum()))
    assert n == 408 and all((query & (kind == k)).any() for k in range(3)) and (~query & (kind >= 0)).any() and (kind < 0).any()
    rng = np.random.RandomState(7)
    g = miro.PhotonMap(200)
    pos = (rng.rand(200, 3) * [4.0, 1.2, 2.0] - [2.0, 0.0, 0.5]).astype(F)
    g.store(np.full((200, 3), 0.01, F), pos, np.tile(np.array([0.0, -1.0, 0.0], F), (200, 1)))
    g.balance()
    seen = []
    for final in (True, False):
        scratch = torch.full((12 * n,), -3.0, dtype=torch.float32, device="cuda")
        rgb = torch.zeros((n, 3), dtype=torch.float32, device="cuda")
        if final:
            scene.final_gather(g, None, rays, hits, n, scratch, rgb, max_dist=1.0, nphotons=20)
        else:
            scene.gather_level(g, None, rays, hits, n, scratch, rgb, d_normal=None, d_weights=None, d_pixels=None, max_dist=1.0, nphotons=20)
        torch.cuda.synchronize()
        seen.append(scratch[:6 * n].cpu().numpy())
    assert np.array_equal(np.isnan(seen[0].reshape(2, n, 3)[1]).all(axis=1), ~query)
    assert seen[0].tobytes() == seen[1].tobytes()
