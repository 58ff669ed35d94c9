"""Reflective bump-mapped materials on the MI355X: a STONE material with ks != 0 on every route (include/miro_hip_bump.h).

Scene::trace bumps the normal of a hit on a STONE material (Scene.cpp:234-263) and Ray::reflect bounces about what it left
(Ray.h:156).  The scene is scenes.photon_room_polished(): the stone room with a floor of ks 0.3 and a wall of ks 0.1.  Yardsticks:

  the generator          a float32 numpy restatement of Ray.h:143-163 (tests/test_bump_specular_plan.py, where it is held to a float64
                         evaluation), fed the device's own normal buffer, the ray and the hit point; bound RTOL / ATOL_OF_MAX of
                         tests/test_procedural.py.  First the plain generator of the parent commit on the mixed room against the same
                         restatement, then the surface form on bumped normals.  On a scene without reflective stone the surface form
                         is the plain generator bit for bit.
  the level kernels      the batched chain trace -> hit_surface -> shade_lights_surface -> gen_secondary_rays_surface on the same
                         queue: per-ray outputs and counters exactly, children as sets, pixel sums within the float-atomic bound --
                         the classes and the comparison of tests/test_level_lights.py.
  the one-call frames    render_specular's batched route on the same renderer arguments: per-level counts exactly, pixels within
                         rtol 1e-5 / atol 1e-6 x max (tests/test_recursion_device.py), bit for bit where a pixel receives one
                         addition per level.
  the photon walk        the host restatement of tests/test_photon_walk_surface.py, record for record.

32 x 24 frames at 1 spp (768 rays: three workgroups of the level kernels), one window of 5 x 3 (15 rays: less than a wave)."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_bump_specular_plan import ATOL_OF_MAX, RTOL, restate_reflect, within  # noqa: E402
from test_frame_lights import MISS, SENTINEL, bits, camera  # noqa: E402
from test_frame_lights_surface import scene_of  # noqa: E402
from test_level_lights import Chain, Fused, assert_level_is_the_chain  # noqa: E402

F = np.float32
PLANE_BIT = np.uint32(0x80000000)
W, H = 32, 24
DEPTH = 3
SEED = 29
LENS = dict(aperture=0.1, focus_plane=5.0)
_OWN = {}


def polished(miro):
    """(scene, description, lights): scenes.photon_room_polished() under the two lights of the other rooms, built once"""
    from miro_amd import scenes
    if "polished" not in _OWN:
        s = miro.Scene(0)
        desc = scenes.textured_room_setup(s, scenes.photon_room_polished())
        _OWN["polished"] = (s, desc, scenes.SCENES["photon_room_two_lights"]["lights"])
    s, desc, lights = _OWN["polished"]
    s.set_lights(lights)
    s.set_environment()
    return s, desc, lights


class Level0:
    """The level-0 queue of a w x h frame at 1 spp with its trace and surface pass, on the device and as numpy rows"""

    def __init__(self, scene, desc, w=W, h=H):
        import torch
        self.n = n = w * h
        f32 = dict(dtype=torch.float32, device="cuda")
        self.rays, self.hits = torch.empty((n, 8), **f32), torch.empty((n, 4), **f32)
        self.color, self.normal = torch.full((n, 3), SENTINEL, **f32), torch.full((n, 3), SENTINEL, **f32)
        scene.gen_eye_rays(camera(desc), w, h, self.rays, spp=1, jitter=False, seed=168)
        scene.trace_device(self.rays, n, self.hits, 0)
        scene.hit_surface(self.rays, self.hits, n, self.color, self.normal)
        torch.cuda.synchronize()
        r, hh = self.rays.cpu().numpy(), self.hits.cpu().numpy()
        self.o, self.d, self.t, self.prim = r[:, 0:3], r[:, 4:7], hh[:, 0], hh[:, 1].copy().view(np.uint32)
        self.N = self.normal.cpu().numpy()
        self.floor = (self.prim != MISS) & ((self.prim & PLANE_BIT) != 0)

    def children(self, scene, surface, octants=True):
        """(count, rays, weights, pixels, octant bytes) of the plain or the surface generator, as numpy, `count` rows each"""
        import torch
        m = 3 * self.n
        out = (torch.full((m, 8), SENTINEL, dtype=torch.float32, device="cuda"), torch.full((m, 3), SENTINEL, dtype=torch.float32, device="cuda"),
               torch.full((m,), 0x7A7A7A7A, dtype=torch.int32, device="cuda"))
        octs = torch.full((m,), 0xEE, dtype=torch.uint8, device="cuda") if octants else None
        count = torch.full((1,), 12345, dtype=torch.int64, device="cuda")
        if surface:
            scene.gen_secondary_rays_surface(self.rays, self.hits, self.normal, None, None, self.n, *out, count, d_out_octants=octs)
        else:
            scene.gen_secondary_rays(self.rays, self.hits, None, None, self.n, *out, count, d_out_octants=octs)
        torch.cuda.synchronize()
        c = int(count.item())
        assert 0 < c <= m
        assert bool((out[0][c:] == SENTINEL).all()) and bool((out[2][c:] == 0x7A7A7A7A).all())      # nothing beyond the count
        return (c,) + tuple(o[:c].cpu().numpy() for o in out) + ((octs[:c].cpu().numpy(),) if octants else ())


def floor_children_against_the_restatement(q, kids, what):
    """The one child (the floor reflects and does not transmit) of every floor hit of q, matched by pixel = ray index, against
    Ray::reflect restated about the device's own normal at P = o + t d.  Returns the largest deviation and the restated
    directions, in the order of np.nonzero(q.floor)."""
    count, rays, weights, pixels = kids[:4]
    idx = np.nonzero(q.floor)[0]
    at = {int(p): [] for p in idx}
    for j, p in enumerate(pixels.tolist()):
        if p in at:
            at[p].append(j)
    assert all(len(v) == 1 for v in at.values()), "a floor hit has exactly one child"
    rows = np.array([at[int(p)][0] for p in idx])
    P = q.o[idx] + q.t[idx, None] * q.d[idx]                              # surface_od's hit point on a plane, in float32
    assert P.dtype == F
    want_o, want_d = restate_reflect(q.d[idx], q.N[idx], P)
    err_d, ok_d = within(rays[rows, 4:7], want_d)
    err_o, ok_o = within(rays[rows, 0:3], want_o)
    print("%s: %d floor hits, largest deviation of the direction %.3g (bound at 1: %.3g), of the origin %.3g" % (
        what, len(idx), err_d.max(), RTOL + ATOL_OF_MAX * np.abs(want_d).max(), err_o.max()))
    assert ok_d and ok_o, (what, err_d.max(), err_o.max())
    assert (rays[rows, 3] == 0).all() and (rays[rows, 7] == F(1e12)).all()
    return max(err_d.max(), err_o.max()), want_d


# ---- 1. the rule -----------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_set_textures_accepts_a_reflective_stone_and_refuses_a_transmitting_one(miro):
    """Fails on the parent commit, which refuses the polished room's table"""
    from miro_amd import binding, scenes
    s, desc, _ = polished(miro)
    assert s.bumped_specular is True and s.procedural
    glassy = list(desc["materials"])
    kd, ks, kt, sh, ri = glassy[0]
    glassy[0] = (kd, ks, (0.1, 0.1, 0.1), sh, ri)
    t = miro.Scene(0)
    scenes.populate(t, desc)
    t.build(4)
    t.set_texcoords(desc["texcoords"], desc["tidx"])
    t.set_materials(glassy, desc["prim_material"])
    with pytest.raises(miro.MiroError) as e:
        t.set_textures(desc["textures"], desc["material_texture"])
    assert e.value.status == binding.MR_ERR_INVALID and "kt" in str(e.value) and "occluder" in str(e.value)
    assert t.bumped_specular is False
    stone, _, _ = scene_of(miro, "stone")
    mixed, _, _ = scene_of(miro, "mixed")
    assert stone.bumped_specular is False and mixed.bumped_specular is False


# ---- 2. the generator on a scene without reflective stone -----------------------------------------------------------------------
@pytest.mark.gpu
def test_the_surface_generator_is_the_plain_one_on_the_mixed_room(miro):
    """count, rays, weights, pixels and octant bytes bit for bit (768 rays are one chunk of the generators: the order is the
    rays').  The mixed room has the glass sphere: reflect, Fresnel and refract children, the Fresnel decision from the buffer's N."""
    s, desc, _ = scene_of(miro, "mixed")
    q = Level0(s, desc)
    a, b = q.children(s, False), q.children(s, True)
    assert a[0] == b[0] and a[0] > 100
    for x, y in zip(a[1:], b[1:]):
        assert x.tobytes() == y.tobytes()
    assert len(np.unique(a[3])) < a[0]                                    # some ray has more than one child


# ---- 3. the generator on bumped normals ---------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_floor_children_bounce_about_the_bumped_normal(miro):
    from miro_amd import binding
    import torch
    mixed, mdesc, _ = scene_of(miro, "mixed")
    qm = Level0(mixed, mdesc)
    assert qm.floor.sum() >= 100
    plain_err, _ = floor_children_against_the_restatement(qm, qm.children(mixed, False), "mr_gen_secondary_rays, mixed room")
    s, desc, _ = polished(miro)
    q = Level0(s, desc)
    kids = q.children(s, True)
    bump_err, want_d = floor_children_against_the_restatement(q, kids, "mr_gen_secondary_rays_surface, polished room")
    # not vacuous: the floor's normals are bumped, and the mirror directions show it by far more than the bound
    idx = np.nonzero(q.floor)[0]
    assert desc["objects"][-1][0] == "plane" and tuple(desc["objects"][-1][1]) == (0.0, 1.0, 0.0)
    plane_n = np.tile(F(desc["objects"][-1][1]), (len(idx), 1))
    bumped = np.abs(q.N[idx] - plane_n).max(axis=1) > 1e-3
    flat_d = restate_reflect(q.d[idx], plane_n, q.o[idx] + q.t[idx, None] * q.d[idx])[1]
    turned = np.abs(want_d - flat_d).max(axis=1)
    print("polished floor: %d hits, %d bumped, directions turned by %.3g (median) .. %.3g; deviations: plain %.3g, surface %.3g" % (
        len(idx), bumped.sum(), np.median(turned), turned.max(), plain_err, bump_err))
    assert bumped.sum() >= 100 and (turned > 1000 * (RTOL + ATOL_OF_MAX)).sum() >= 100
    # the two calls that compute the object's own normal refuse the scene and name the call that does not
    m = 3 * q.n
    out = (torch.empty((m, 8), dtype=torch.float32, device="cuda"), torch.empty((m, 3), dtype=torch.float32, device="cuda"),
           torch.empty(m, dtype=torch.int32, device="cuda"))
    count = torch.zeros(1, dtype=torch.int64, device="cuda")
    with pytest.raises(miro.MiroError) as e:
        s.gen_secondary_rays(q.rays, q.hits, None, None, q.n, *out, count)
    assert e.value.status == binding.MR_ERR_STATE and "mr_gen_secondary_rays_surface" in str(e.value)
    with pytest.raises(miro.MiroError) as e:
        s.gen_path_rays(q.rays, q.hits, None, None, None, q.n, *out, None, count, kinds=binding.MR_PATH_MIRROR)
    assert e.value.status == binding.MR_ERR_STATE and "mr_gen_path_rays_surface" in str(e.value)
    s.gen_path_rays(q.rays, q.hits, None, None, None, q.n, *out, None, count, kinds=binding.MR_PATH_REFRACT)   # only the mirror lobe is refused
    torch.cuda.synchronize()
    # NULL and misaligned d_normal: MR_ERR_INVALID, after the plain call's own list
    L = miro.lib()
    args = lambda normal: (s.h, q.rays.data_ptr(), q.hits.data_ptr(), normal, None, None, q.n, 1, out[0].data_ptr(), out[1].data_ptr(),  # noqa: E731
                           out[2].data_ptr(), count.data_ptr(), m, None, None)
    for normal in (None, q.normal.data_ptr() + 2):
        assert L.mr_gen_secondary_rays_surface(*args(normal)) == binding.MR_ERR_INVALID and b"d_normal" in L.mr_last_error()


# ---- 4. the level kernel ------------------------------------------------------------------------------------------------------
class SurfaceChain(Chain):
    """tests/test_level_lights.py's chain with the children of gen_secondary_rays_surface, fed the chain's own normal buffer"""

    def __init__(self, scene, n_lights, rays, weights, pixels, n, spp, flags, env, children, n_pixels):
        import torch
        super().__init__(scene, n_lights, rays, weights, pixels, n, spp, flags, env, False, n_pixels)
        if children:
            out = (torch.empty((3 * n, 8), dtype=torch.float32, device="cuda"), torch.empty((3 * n, 3), dtype=torch.float32, device="cuda"),
                   torch.empty(3 * n, dtype=torch.int32, device="cuda"))
            count = torch.zeros(1, dtype=torch.int64, device="cuda")
            scene.gen_secondary_rays_surface(rays, self.hits, self.normal, weights, pixels, n, *out, count, spp=spp)
            torch.cuda.synchronize()
            self.n_children = int(count.item())
            self.out = tuple(o[:self.n_children].contiguous() for o in out)


@pytest.mark.gpu
@pytest.mark.parametrize("window", [(W, H), (5, 3)], ids=["32x24", "5x3"])
def test_trace_level_lights_is_the_chain_on_the_polished_room(miro, window):
    """Levels 0 to 3 on the same queues, the chain's queue feeding the next level, every level WITH children (the BUMPED kernels);
    at 5 x 3 level 0 alone.  Hit records, colour, normal, per-ray L and the five counters on their bits, the children as sets, the
    pixel sums within the float-atomic bound.  Children of floor hits occur at every level that has rays."""
    import torch
    from miro_amd import binding
    s, desc, lights = polished(miro)
    w, h = window
    n = w * h
    rays = torch.empty((n, 8), dtype=torch.float32, device="cuda")
    s.gen_eye_rays(camera(desc), w, h, rays, spp=1, jitter=False, seed=168)
    weights = pixels = None
    for level in range(DEPTH + 1 if window == (W, H) else 1):
        flags = binding.MR_TRACE_INCOHERENT if level > 0 else 0
        ch = SurfaceChain(s, len(lights), rays, weights, pixels, n, 1, flags, None, True, w * h)
        fu = Fused(s, rays, weights, pixels, n, 1, flags, None, True, w * h)
        prim = ch.hits[:, 1].contiguous().view(torch.int32).cpu().numpy().view(np.uint32)
        floor = (prim != MISS) & ((prim & PLANE_BIT) != 0)
        print("%dx%d level %d: %d rays, %d hits (%d on the floor), %d children, counters %s" % (
            w, h, level, n, ch.n_hits, floor.sum(), ch.n_children, ch.counted))
        assert_level_is_the_chain(fu, ch)
        assert n > 0 and ch.n_children >= floor.sum() and (floor.sum() > 0 or window != (W, H))
        kid_pixels = set(ch.out[2].cpu().numpy().tolist())
        parent_pixels = np.arange(n) if pixels is None else pixels.cpu().numpy()
        assert set(parent_pixels[floor].tolist()) <= kid_pixels          # every floor hit's pixel has a child in the next queue
        rays, weights, pixels, n = ch.out[0], ch.out[1], ch.out[2], ch.n_children
    stone, sdesc, slights = scene_of(miro, "stone")                       # a scene without the flag keeps the plain kernels: its chain
    stone.set_environment()
    rays = torch.empty((W * H, 8), dtype=torch.float32, device="cuda")
    stone.gen_eye_rays(camera(sdesc), W, H, rays, spp=1, jitter=False, seed=168)
    assert_level_is_the_chain(Fused(stone, rays, None, None, W * H, 1, 0, None, True, W * H),
                              Chain(stone, len(slights), rays, None, None, W * H, 1, 0, None, True, W * H))


# ---- 5. the one-call frames ---------------------------------------------------------------------------------------------------
def frame_of(miro, fused, spp=1, lens=None, **kw):
    """One render_specular frame of the polished room at depth 3; returns the renderer with per_level, rgb and, on the batched
    route, the pixel column of every queue of levels >= 1"""
    import torch
    from miro_amd import frame

    class Spy(frame.FrameRenderer):
        def _level_batched(self, plan, q, level, last):
            if level > 0:
                self.seen_pixels.append(q.pixels)
            return super()._level_batched(plan, q, level, last)

    s, desc, lights = polished(miro)
    queue = fused in (False, "lights")                  # the routes that read the eye rays from the renderer's resident queue
    fr = Spy(s, desc, W, H, spp=spp, tiled=False, lens=lens, resident_rays=queue)
    fr.seen_pixels = []
    if queue:
        fr.generate()
    if isinstance(fused, str) and fused.startswith("device_"):
        kw = dict(kw, queue_capacity=4 ** DEPTH * W * H * spp)             # fan^depth x the samples: no level can truncate
    fr.per_level = fr.render_specular(depth=DEPTH, lights=lights, fused=fused, **kw)
    torch.cuda.synchronize()
    fr.rgb = fr.d_rgb.clone()
    fr.pixels = [p.cpu().numpy() for p in fr.seen_pixels]
    return fr


def assert_pixels_close(got, want):
    import torch
    scale = float(want.abs().max())
    assert scale > 0
    assert torch.allclose(got, want, rtol=1e-5, atol=1e-6 * scale), float((got - want).abs().max())


@pytest.mark.gpu
def test_one_call_frame_against_the_level_route_and_the_batched_route(miro):
    """fused="device_lights" (mr_render_recursion: the queued BUMPED kernels) against fused="lights" (mr_trace_level_lights per
    level) and fused=False (the chain with gen_secondary_rays_surface), depth 3: per-level counts exactly; pixels within the
    bound, and on their bits where a pixel receives one addition per level -- read from the batched route's own queues."""
    ref = frame_of(miro, False)
    lev = frame_of(miro, "lights")
    dev = frame_of(miro, "device_lights")
    print("per_level", ref.per_level)
    assert len(ref.per_level) == DEPTH + 1 and all(n > 0 for n, _ in ref.per_level)
    assert dev.per_level == lev.per_level == ref.per_level
    assert_pixels_close(dev.rgb, ref.rgb)
    assert_pixels_close(dev.rgb, lev.rgb)
    assert_pixels_close(lev.rgb, ref.rgb)
    once = np.ones(W * H, bool)
    assert len(ref.pixels) == DEPTH
    for p in ref.pixels:
        once &= np.bincount(p.astype(np.int64), minlength=W * H) <= 1
    print("%d of %d pixels receive one addition per level" % (once.sum(), W * H))
    assert once.sum() >= 100
    sel = np.nonzero(once)[0]
    assert np.array_equal(bits(dev.rgb)[sel], bits(ref.rgb)[sel]) and np.array_equal(bits(lev.rgb)[sel], bits(ref.rgb)[sel])


@pytest.mark.gpu
def test_one_call_frame_through_the_lens_at_four_samples(miro):
    ref = frame_of(miro, False, spp=4, lens=LENS)
    dev = frame_of(miro, "device_lens", spp=4, lens=LENS)
    assert len(ref.per_level) == DEPTH + 1 and dev.per_level == ref.per_level and ref.per_level[0][0] == W * H * 4
    assert_pixels_close(dev.rgb, ref.rgb)


@pytest.mark.gpu
@pytest.mark.parametrize("fused", ["device_lights_path", "frame_lights_path"])
def test_the_path_routes_accept_the_scene(miro, fused):
    """the PATH kernels took the surface step's normal before: they accept the polished room and agree with the batched path
    route on gen_path_rays_surface"""
    kw = dict(path_tracing=True, path_kinds=7, path_seed=SEED)
    ref = frame_of(miro, False, surface_children=True, **kw)
    got = frame_of(miro, fused, **kw)
    assert len(ref.per_level) == DEPTH + 1 and got.per_level == ref.per_level
    assert_pixels_close(got.rgb, ref.rgb)
    with pytest.raises(ValueError):
        frame_of(miro, False, surface_children=False, **kw)


# ---- 6. the photon walk -------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_photon_walk_on_the_polished_room_is_the_restatements(oracle, miro):
    """mr_trace_photons_surface, caustic photons (a first mirror event on the floor keeps the photon alive): emitted, stored,
    segments, the records and the balanced map are the host restatement's, whose mirror event reflects about the surface pass's
    normal -- the bumped one on the polished floor and wall."""
    from test_photon_walk_surface import check_surface_against_restatement, product_textured_room, textured_walker
    from miro_amd import scenes
    desc = scenes.photon_room_polished()
    scene = product_textured_room(miro, desc)
    assert scene.bumped_specular is True
    w = textured_walker(oracle, scene, desc, True)
    want = check_surface_against_restatement(oracle, miro, scene, desc, w, 1500, 40000, True)
    print("emitted %d, stored %d; events %s; stores per material %s" % (want["emitted"], want["stored"], w.events, w.stores_by_mat.tolist()))
    assert want["stored"] >= 1500 and w.events["mirror"] > 100
