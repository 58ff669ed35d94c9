"""mr_gen_path_rays_surface (csrc/mr_path_surface.hip, body in csrc/mr_children_body.h) -- the PATH_TRACING generators with every
hit's N and the diffuse child's colour read from the two buffers of mr_hit_surface, the form of mr_gen_path_rays for a scene
with a texture table.

Three checkers, none of them the code under test:
  * mr_gen_path_rays itself, which tests/test_path_rays.py holds to the oracle bit for bit: on an untextured scene the buffers
    hold the object's normal and the material's colour, so the two calls must write the same bytes; and fed the buffers of a
    twin scene with other vertex normals and other diffuse colours, the surface call must write what the plain call writes on
    that twin.
  * ray_random of tests/test_photon_walk_surface.py, Ray::random about an arbitrary normal in numpy float32, which
    test_numpy_ray_random_is_the_oracles_diffuse_child holds to the oracle bit for bit; the diffuse child's weight is the
    float32 product w0 * colour.
  * the same launches made by hand, for FrameRenderer.render_specular.
Queues are compared as sets (the order across chunks of kGenIter * kBlock = 2 048 rays is decided by an atomic), records as
bytes.  Pixel sums of multi-bounce frames: rtol 1e-5, atol 1e-6 x max, the bound of tests/test_level.py for the order of float
atomics."""
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import kernel_budget  # noqa: E402
from test_photon_walk import pcg32, product_room, unit01  # noqa: E402,F401
from test_photon_walk_surface import normalised, product_textured_room, ray_random  # noqa: E402

F = np.float32
NAME = "mr_gen_path_rays_surface"
MISS = 0xFFFFFFFF
PLANE_BIT = 0x80000000
CHUNK = 2048                                                   # kGenIter * kBlock
SENTINEL, SENTINEL_INT, SENTINEL_OCT = 12345.0, 77, 0xEE
ALL_KINDS = 7


def child_id(ids, kind):
    """rec::child_id (csrc/mr_recursion.h): pcg32(id ^ (0x9e3779b9 * (kind + 1)))"""
    return pcg32(np.asarray(ids, np.uint32) ^ np.uint32((0x9e3779b9 * (kind + 1)) & 0xFFFFFFFF))


# ---- without a GPU -------------------------------------------------------------------------------------------------------
def test_the_surface_path_entry_is_exported_and_declared_outside_miro_hip_h(miro):
    from miro_amd import binding
    L = miro.lib()

    def declared(header):
        src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
        return re.search(r"\b%s\s*\(" % NAME, src) is not None

    assert hasattr(L, NAME) and NAME in binding.SURFACE_SYMBOLS and NAME not in miro.EXPORTED_SYMBOLS
    assert declared("miro_hip_surface.h") and not declared("miro_hip.h")
    assert NAME in open(os.path.join(ROOT, "include", "miro_hip.h")).read()                  # documented there
    assert hasattr(miro.Scene, "gen_path_rays_surface")


def test_path_surface_kernel_stays_inside_the_verified_envelope():
    """The one kernel of mr_path_surface.hip: no dynamic stack; no more spilled VGPRs, no more scratch per lane and no fewer waves
    per SIMD than BOTH its own record (tests/golden/kernel_budget_path_surface.json, written from the build whose GPU run of this
    file was green) AND the worst value among the kernels of tests/golden/kernel_budget.json."""
    cur = kernel_budget.unit_kernels("mr_path_surface")
    assert len(cur) == 1 and all("children_surf_kernel" in k for k in cur)
    kernel_budget.assert_inside_envelope(cur, "kernel_budget_path_surface.json")


# ---- on the MI355X: helpers ------------------------------------------------------------------------------------------------
def cuda(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def ray_records(miro, o, d):
    r = np.zeros(len(o), miro.RAY_DTYPE)
    r["ox"], r["oy"], r["oz"], r["tmin"] = o[:, 0], o[:, 1], o[:, 2], 0.0
    r["dx"], r["dy"], r["dz"], r["tmax"] = d[:, 0], d[:, 1], d[:, 2], 1e12
    return r


class Batch:
    """n rays traced against a scene: device rays and hits, host hit records"""

    def __init__(self, miro, scene, rays):
        import torch
        self.miro, self.scene, self.n = miro, scene, len(rays)
        self.rays_np = rays
        self.rays = cuda(rays.view(F).reshape(self.n, 8).copy())
        self.hits = torch.empty((self.n, 4), dtype=torch.float32, device="cuda")
        scene.trace_device(self.rays, self.n, self.hits)
        torch.cuda.synchronize()
        self.hits_np = self.hits.cpu().numpy().view(miro.HIT_DTYPE).reshape(-1)
        self.prim = self.hits_np["prim"]
        self.hit = self.prim != MISS

    def surface(self, scene=None):
        """(d_color, d_normal) of mr_hit_surface on `scene` (default: the batch's own); the rows of a miss hold NaN"""
        import torch
        color = torch.full((self.n, 3), float("nan"), dtype=torch.float32, device="cuda")
        normal = torch.full((self.n, 3), float("nan"), dtype=torch.float32, device="cuda")
        (scene or self.scene).hit_surface(self.rays, self.hits, self.n, color, normal)
        torch.cuda.synchronize()
        return color, normal

    def attrs(self):
        """(P, N as HitInfo holds it) of mr_hit_attrs, [n, 3] each"""
        import torch
        P = torch.empty((self.n, 3), dtype=torch.float32, device="cuda")
        N = torch.empty((self.n, 3), dtype=torch.float32, device="cuda")
        self.scene.hit_attrs(self.hits, self.n, P, N, d_rays=self.rays)
        torch.cuda.synchronize()
        return P.cpu().numpy(), N.cpu().numpy()


class Queue:
    """A child queue of 4n slots (+ `capacity` given to the call), pre-filled with sentinels, as numpy after the call"""

    def __init__(self, batch, scene, surface, kinds=ALL_KINDS, w=None, pix=None, ids=None, spp=1, seed=168, bounce=0, capacity=None,
                 octants=True):
        import torch
        n = batch.n
        room = 4 * n
        rays = torch.full((room, 8), SENTINEL, dtype=torch.float32, device="cuda")
        wgt = torch.full((room, 3), SENTINEL, dtype=torch.float32, device="cuda")
        pixels = torch.full((room,), SENTINEL_INT, dtype=torch.int32, device="cuda")
        cids = torch.full((room,), SENTINEL_INT, dtype=torch.int32, device="cuda")
        octs = torch.full((room,), SENTINEL_OCT, dtype=torch.uint8, device="cuda") if octants else None
        cnt = torch.full((1,), -1, dtype=torch.int64, device="cuda")
        kw = dict(spp=spp, seed=seed, bounce=bounce, kinds=kinds, out_capacity=room if capacity is None else capacity, d_out_octants=octs)
        if surface is None:
            scene.gen_path_rays(batch.rays, batch.hits, w, pix, ids, n, rays, wgt, pixels, cids, cnt, **kw)
        else:
            scene.gen_path_rays_surface(batch.rays, batch.hits, surface[0], surface[1], w, pix, ids, n, rays, wgt, pixels, cids, cnt, **kw)
        torch.cuda.synchronize()
        self.count = int(cnt.item())
        self.rays = rays.cpu().numpy().view(np.uint32)
        self.w = wgt.cpu().numpy()
        self.pix = pixels.cpu().numpy().view(np.uint32)
        self.ids = cids.cpu().numpy().view(np.uint32)
        self.oct = octs.cpu().numpy() if octants else np.zeros(room, np.uint8)

    def rows(self, m=None):
        """slots [0, m) as rows of uint32 (id first), in lexicographic order"""
        m = self.count if m is None else m
        t = np.concatenate([self.ids[:m, None], self.rays[:m], self.w[:m].view(np.uint32), self.pix[:m, None],
                            self.oct[:m, None].astype(np.uint32)], axis=1)
        return t[np.lexsort(t.T[::-1])]

    def untouched(self, m):
        """slots [m, 4n) still hold the sentinels"""
        return bool((self.rays[m:].view(F) == SENTINEL).all() and (self.w[m:] == SENTINEL).all() and (self.pix[m:] == SENTINEL_INT).all()
                    and (self.ids[m:] == SENTINEL_INT).all() and (self.oct[m:] == SENTINEL_OCT).all())


def room_rays(miro, n, seed, miss_share=0.2):
    """Rays from inside photon_room in seeded directions (the room is closed: each hits something); a share of them moved outside
    and aimed away, above the floor plane, so that they miss."""
    rng = np.random.RandomState(seed)
    o = np.stack([rng.uniform(-1.5, 1.5, n), rng.uniform(0.3, 3.5, n), rng.uniform(-1.5, 1.5, n)], 1).astype(F)
    d = rng.randn(n, 3)
    d = (d / np.linalg.norm(d, axis=1)[:, None]).astype(F)
    out = rng.rand(n) < miss_share
    o[out] = np.array([10.0, 10.0, 10.0], F)
    d[out] = np.abs(d[out])
    return ray_records(miro, o, d)


# ---- 3. plain scenes reproduce mr_gen_path_rays ----------------------------------------------------------------------------
N_PLAIN = CHUNK + 515                                          # one full chunk and a partial one


@pytest.fixture(scope="module")
def room(miro):
    scene, _ = product_room(miro, "photon_room")
    return Batch(miro, scene, room_rays(miro, N_PLAIN, 5))


@pytest.mark.gpu
@pytest.mark.parametrize("kinds", [1, 2, 3, 4, 5, 6, 7])
def test_untextured_room_reproduces_the_plain_call(room, kinds):
    """photon_room (diffuse walls, a slightly glossy floor plane, a glass and a mirror sphere), 2 048 + 515 rays of which about a
    fifth miss; the buffers are NaN wherever mr_hit_surface did not write.  Rays, weights, pixels, ids, octant bytes and *d_count
    equal mr_gen_path_rays' bytes (as sets of records) with explicit weights / pixels / ids at bounce 0 and 3 and with all three
    NULL; no output is NaN; nothing beyond the count is written."""
    n = room.n
    color, normal = room.surface()
    assert 0.1 * n < (~room.hit).sum() < 0.3 * n
    assert np.isnan(color.cpu().numpy()[~room.hit]).all() and np.isnan(normal.cpu().numpy()[~room.hit]).all()
    assert np.isfinite(color.cpu().numpy()[room.hit]).all() and np.isfinite(normal.cpu().numpy()[room.hit]).all()
    rng = np.random.RandomState(17)
    w = cuda(rng.rand(n, 3).astype(F))
    pix = cuda(rng.randint(0, 1000, n).astype(np.int32))
    ids = cuda(rng.randint(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32).view(np.int32))
    total = 0
    for args in (dict(w=w, pix=pix, ids=ids, bounce=0), dict(w=w, pix=pix, ids=ids, bounce=3, seed=9), dict(spp=2)):
        want = Queue(room, room.scene, None, kinds=kinds, **args)
        got = Queue(room, room.scene, (color, normal), kinds=kinds, **args)
        assert got.count == want.count and 0 < got.count <= 4 * n
        assert got.untouched(got.count) and want.untouched(want.count)
        a, b = got.rows(), want.rows()
        assert not np.isnan(got.w[:got.count]).any() and not np.isnan(got.rays[:got.count].view(F)).any()
        assert a.tobytes() == b.tobytes()
        total += got.count
    print("kinds %d: %d children of %d hits in three calls" % (kinds, total, room.hit.sum()))
    if kinds == ALL_KINDS:
        assert total > 3 * room.hit.sum()                      # some hits have several children


# ---- 4. / 5. twin scenes: only the buffers are read --------------------------------------------------------------------------
GRID = 6                                                        # GRID x GRID quads in the plane z = 0
TWIN_KS_KT = [((0.3, 0.2, 0.1), (0.0, 0.0, 0.0), 30.0, 1.0), ((0.1, 0.1, 0.1), (0.5, 0.6, 0.7), 200.0, 1.5),
              ((0.0, 0.0, 0.0), (0.0, 0.0, 0.0), float("inf"), 1.0)]


def twin_scene(miro, turned, kd_seed):
    """GRID x GRID x 2 triangles in the plane z = 0, material = triangle index mod 3: glossy mirror, rough glass, Lambert, each
    with a diffuse colour drawn from kd_seed.  turned: every vertex normal is the face normal (0, 0, 1) turned by a seeded angle
    of up to 0.3 rad; otherwise flat."""
    s = miro.Scene(0)
    rng = np.random.RandomState(23)
    tris = []
    for j in range(GRID):
        for i in range(GRID):
            x0, y0, x1, y1 = i - GRID / 2, j - GRID / 2, i + 1 - GRID / 2, j + 1 - GRID / 2
            tris.append([x0, y0, 0, x1, y0, 0, x1, y1, 0])
            tris.append([x0, y0, 0, x1, y1, 0, x0, y1, 0])
    for t in tris:
        normals = np.tile(np.array([0.0, 0.0, 1.0]), 3).reshape(3, 3)
        if turned:
            ang, az = rng.uniform(0.0, 0.3, 3), rng.uniform(0.0, 2 * np.pi, 3)
            normals = np.stack([np.sin(ang) * np.cos(az), np.sin(ang) * np.sin(az), np.cos(ang)], 1)
        s.add_triangle(np.asarray(t, F), normals.astype(F).reshape(9))
    kd = np.random.RandomState(kd_seed).uniform(0.02, 0.2, (3, 3))
    s.set_materials([(tuple(kd[m]), ks, kt, sh, ix) for m, (ks, kt, sh, ix) in enumerate(TWIN_KS_KT)], np.arange(len(tris)) % 3)
    s.build(4)
    return s


def twin_rays(miro, n):
    """Rays onto the grid from both sides (a refractive hit is entered and left), a share of them aimed past it"""
    rng = np.random.RandomState(29)
    target = np.stack([rng.uniform(-GRID / 2 - 0.6, GRID / 2 + 0.6, n), rng.uniform(-GRID / 2 - 0.6, GRID / 2 + 0.6, n), np.zeros(n)], 1)
    o = np.stack([rng.uniform(-3, 3, n), rng.uniform(-3, 3, n), rng.uniform(1.0, 4.0, n) * np.where(rng.rand(n) < 0.3, -1.0, 1.0)], 1)
    d = target - o
    d /= np.linalg.norm(d, axis=1)[:, None]
    return ray_records(miro, o.astype(F), d.astype(F))


@pytest.fixture(scope="module")
def twins(miro):
    a, b = twin_scene(miro, False, 31), twin_scene(miro, True, 37)
    rays = twin_rays(miro, N_PLAIN)
    A, B = Batch(miro, a, rays), Batch(miro, b, rays)
    assert A.hits_np.tobytes() == B.hits_np.tobytes()          # the same triangles: the same hits
    assert 0.05 * A.n < (~A.hit).sum() < 0.5 * A.n
    return A, B


@pytest.mark.gpu
def test_only_the_buffers_are_read(twins):
    """Scene A (flat normals, its own kd) fed mr_hit_surface's buffers computed on scene B (turned vertex normals, other kd)
    writes what mr_gen_path_rays writes on B, byte for byte, for all three kinds on triangles with ks, kt and kd -- and not what
    it writes on A."""
    A, B = twins
    n = A.n
    rng = np.random.RandomState(41)
    w = cuda(rng.rand(n, 3).astype(F))
    ids = cuda(rng.randint(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32).view(np.int32))
    surface_b = B.surface()
    for bounce in (0, 2):
        want = Queue(B, B.scene, None, w=w, ids=ids, bounce=bounce)
        got = Queue(A, A.scene, surface_b, w=w, ids=ids, bounce=bounce)
        own = Queue(A, A.scene, None, w=w, ids=ids, bounce=bounce)
        assert got.count == want.count > A.hit.sum() and got.untouched(got.count)
        a, b = got.rows(), want.rows()
        kinds_seen = {k for k in range(4) if np.isin(child_id(ids.cpu().numpy().view(np.uint32)[A.hit], k), got.ids[:got.count]).any()}
        print("bounce %d: %d children of %d hits, kinds %s; %d rows differ from scene A's own call" % (
            bounce, got.count, A.hit.sum(), sorted(kinds_seen), (a != own.rows()[:len(a)]).any(axis=1).sum() if own.count == got.count else -1))
        assert kinds_seen == {0, 1, 2, 3}
        assert a.tobytes() == b.tobytes()
        assert own.count != got.count or own.rows().tobytes() != a.tobytes()


@pytest.mark.gpu
@pytest.mark.parametrize("bounce,seed", [(0, 168), (3, 7)])
def test_diffuse_child_is_ray_random_about_the_buffered_normal(oracle, twins, bounce, seed):
    """Scene A with a seeded colour in [0, 1)^3 per ray and the geometric normal turned by up to 0.3 rad (normalised in float32):
    the diffuse children (id == child_id(id, 3)) are ray_random(N_buf, P of mr_hit_attrs) bit for bit, origin and direction, and
    carry the float32 products w0 * colour bit for bit."""
    A, _ = twins
    n = A.n
    rng = np.random.RandomState(43)
    P, N = A.attrs()
    idx = np.nonzero(A.hit)[0]
    Ng = normalised(N[idx]).astype(np.float64)
    t = np.cross(Ng, rng.randn(len(idx), 3))
    t /= np.linalg.norm(t, axis=1)[:, None]
    ang = rng.uniform(0.0, 0.3, len(idx))
    turned = normalised((Ng * np.cos(ang)[:, None] + t * np.sin(ang)[:, None]).astype(F))
    color_np, normal_np = np.full((n, 3), np.nan, F), np.full((n, 3), np.nan, F)
    color_np[idx], normal_np[idx] = rng.rand(len(idx), 3).astype(F), turned
    w_np = rng.rand(n, 3).astype(F)
    ids_np = rng.randint(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    got = Queue(A, A.scene, (cuda(color_np), cuda(normal_np)), w=cuda(w_np), ids=cuda(ids_np.view(np.int32)), bounce=bounce, seed=seed)
    m = got.count
    assert m > len(idx) and got.untouched(m)
    want_id = child_id(ids_np[idx], 3)                          # every material of A is diffuse: one such child per hit
    order = np.argsort(got.ids[:m], kind="stable")
    at = np.searchsorted(got.ids[:m][order], want_id)
    assert (at < m).all()
    slot = order[np.minimum(at, m - 1)]
    assert np.array_equal(got.ids[slot], want_id) and len(np.unique(slot)) == len(idx)
    org, dr = ray_random(oracle, turned, P[idx], ids_np[idx], bounce, pcg32(np.uint32(seed)))
    rays = got.rays[slot].view(F)
    assert rays[:, 4:7].tobytes() == dr.tobytes() and rays[:, 0:3].tobytes() == org.tobytes()
    assert (rays[:, 3] == 0).all() and (rays[:, 7] == F(1e12)).all()
    assert got.w[slot].tobytes() == (w_np[idx] * color_np[idx]).astype(F).tobytes()
    flat_org, flat_dir = ray_random(oracle, normalised(N[idx]), P[idx], ids_np[idx], bounce, pcg32(np.uint32(seed)))
    assert (flat_dir != dr).any(axis=1).mean() > 0.9            # the buffered normal matters
    assert not np.isnan(got.w[:m]).any() and not np.isnan(got.rays[:m].view(F)).any()


# ---- 6. slot accounting -----------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_slot_accounting_on_a_glass_sphere(miro):
    """A glass sphere (kd = 0, ks, kt) hit by parallel rays from normal to grazing incidence, so that Rs falls on both sides of
    0.01 and a parent has 2 or 3 children.  Pass 1 counts from the buffered N and pass 2 generates from it: every slot in
    [0, count) is written once (no sentinel left, `count` distinct ids, each parent's 2 or 3), a parent's children are adjacent,
    nothing in [count, 4n) is touched.  With out_capacity = count - 5: *d_count still the full count, every slot below the capacity
    written with one of the full run's children, everything from the capacity on untouched."""
    s = miro.Scene(0)
    s.add_triangle([40, 0, 40, 41, 0, 40, 40, 1, 40], [0, 0, 1] * 3)                          # far away: a scene needs one bounded object
    s.add_sphere((0.0, 0.0, 0.0), 1.0)
    s.set_materials([((0.5, 0.5, 0.5), (0, 0, 0), (0, 0, 0), 1.0, 1.0), ((0.0, 0.0, 0.0), (0.05, 0.05, 0.05), (0.9, 0.9, 0.9), 80.0, 1.5)], [0, 1])
    s.build(4)
    n = CHUNK + 700
    rng = np.random.RandomState(47)
    r = np.sqrt(rng.rand(n)) * 1.05                              # impact parameter: a few rays pass the sphere
    az = rng.uniform(0, 2 * np.pi, n)
    o = np.stack([r * np.cos(az), r * np.sin(az), np.full(n, 5.0)], 1).astype(F)
    d = np.tile(np.array([0.0, 0.0, -1.0], F), (n, 1))
    b = Batch(miro, s, ray_records(miro, o, d))
    surface = b.surface()
    full = Queue(b, s, surface)
    m = full.count
    hit = np.nonzero(b.hit)[0]
    assert 0 < (~b.hit).sum() < n // 4 and (b.prim[hit] == 1).all()
    per_parent = np.bincount(full.pix[:m], minlength=n)         # pixels NULL, spp 1: a child's pixel is its parent's index
    print("glass sphere: %d hits, %d children; parents with 2 children %d, with 3 %d" % (len(hit), m, (per_parent == 2).sum(), (per_parent == 3).sum()))
    assert (per_parent[~b.hit] == 0).all() and set(np.unique(per_parent[hit])) == {2, 3}
    assert (per_parent == 2).sum() > 50 and (per_parent == 3).sum() > 50
    assert m == per_parent.sum() and full.untouched(m)
    assert (full.rays[:m].view(F)[:, 7] == F(1e12)).all() and (full.w[:m] != SENTINEL).all()
    assert len(np.unique(full.ids[:m])) == m
    for kind, expect in ((0, hit), (2, hit), (1, np.nonzero(per_parent == 3)[0])):
        assert np.isin(child_id(expect, kind), full.ids[:m]).all(), kind
    assert not np.isin(child_id(np.nonzero(per_parent == 2)[0], 1), full.ids[:m]).any()
    runs = 1 + int((full.pix[1:m] != full.pix[:m - 1]).sum())
    assert runs == len(hit)                                     # each parent's children next to one another
    plain = Queue(b, s, None)
    assert plain.count == m and plain.rows().tobytes() == full.rows().tobytes()
    cap = m - 5
    part = Queue(b, s, surface, capacity=cap)
    assert part.count == m and part.untouched(cap)
    assert (part.rays[:cap].view(F)[:, 7] == F(1e12)).all() and (part.w[:cap] != SENTINEL).all()
    assert len(np.unique(part.ids[:cap])) == cap and np.isin(part.ids[:cap], full.ids[:m]).all()
    by_id = {int(row[0]): row.tobytes() for row in full.rows()}
    assert all(by_id[int(row[0])] == row.tobytes() for row in part.rows(cap))


# ---- 7. the stone room -------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def stone(miro):
    from miro_amd import scenes
    desc = scenes.photon_room_stone()
    return product_textured_room(miro, desc), desc


def eye_batch(miro, scene, desc, W, H):
    import torch
    from miro_amd import binding
    d_rays = torch.empty((W * H, 8), dtype=torch.float32, device="cuda")
    scene.gen_eye_rays(binding.make_camera(desc["eye"], desc["lookat"], desc["up"], desc["fov"]), W, H, d_rays)
    torch.cuda.synchronize()
    return Batch(miro, scene, d_rays.cpu().numpy().view(miro.RAY_DTYPE).reshape(-1))


@pytest.mark.gpu
def test_stone_floor_bounces_about_the_bumped_normal(oracle, miro, stone):
    """photon_room_stone() at 24 x 16 eye rays: the diffuse children of floor hits are ray_random about mr_hit_surface's normal,
    bit for bit, and at least half of them differ from ray_random about mr_hit_attrs' normalised normal; their weight is the
    stone colour.  mr_gen_path_rays on the scene still returns MR_ERR_STATE, and its message names mr_gen_path_rays_surface."""
    from miro_amd import binding
    scene, desc = stone
    b = eye_batch(miro, scene, desc, 24, 16)
    assert scene.procedural
    color, normal = b.surface()
    got = Queue(b, scene, (color, normal))
    m = got.count
    P, N = b.attrs()
    floor = np.nonzero(b.hit & ((b.prim & np.uint32(PLANE_BIT)) != 0))[0]
    assert len(floor) > b.n // 8
    want_id = child_id(floor, 3)                                # ids NULL: a ray's id is its index
    order = np.argsort(got.ids[:m], kind="stable")
    slot = order[np.minimum(np.searchsorted(got.ids[:m][order], want_id), m - 1)]
    assert np.array_equal(got.ids[slot], want_id)
    bumped = normal.cpu().numpy()[floor]
    org, dr = ray_random(oracle, bumped, P[floor], floor.astype(np.uint32), 0, pcg32(np.uint32(168)))
    _, flat_dir = ray_random(oracle, normalised(N[floor]), P[floor], floor.astype(np.uint32), 0, pcg32(np.uint32(168)))
    rays = got.rays[slot].view(F)
    differ = (flat_dir != dr).any(axis=1).mean()
    print("stone room: %d rays, %d on the floor, %d children; share of floor children that the flat normal sends elsewhere %.3f" % (
        b.n, len(floor), m, differ))
    assert rays[:, 4:7].tobytes() == dr.tobytes() and rays[:, 0:3].tobytes() == org.tobytes()
    assert differ >= 0.5
    assert got.w[slot].tobytes() == color.cpu().numpy()[floor].tobytes()                      # w0 = 1
    assert not np.isnan(got.w[:m]).any() and got.untouched(m)
    with pytest.raises(miro.MiroError) as e:
        Queue(b, scene, None)
    assert e.value.status == binding.MR_ERR_STATE == -5 and NAME in str(e.value)
    assert Queue(b, scene, None, kinds=3).rows().tobytes() == Queue(b, scene, (color, normal), kinds=3).rows().tobytes()


# ---- 8. frames ---------------------------------------------------------------------------------------------------------------
def record_calls(scene, names, calls):
    for name in names:
        def wrap(f, name=name):
            def g(*a, **k):
                calls.append((name, a, k))
                return f(*a, **k)
            return g
        setattr(scene, name, wrap(getattr(scene, name)))


def frame_by_hand(torch, fr, scene, depth, kinds, queues):
    """render_specular(depth, path_tracing=True, path_kinds=kinds, lights=...) on a scene with a procedural texture, launch by
    launch; queues: receives (n, out_rays, out_w, out_pix, out_ids, count) per generating level"""
    from miro_amd import binding
    f32 = dict(dtype=torch.float32, device="cuda")
    rgb = torch.zeros((fr.n_pixels, 3), **f32)
    rays, weights, pixels, ids, n = fr.d_rays, None, None, None, fr.n
    per_level = []
    for level in range(depth + 1):
        if n == 0:
            break
        fl = fr.flags | (binding.MR_TRACE_INCOHERENT if level > 0 else 0)
        hits, color, normal = torch.empty((n, 4), **f32), torch.empty((n, 3), **f32), torch.empty((n, 3), **f32)
        cnt = torch.zeros(1, dtype=torch.int64, device="cuda")
        scene.trace_device(rays, n, hits, fl)
        scene.hit_surface(rays, hits, n, color, normal)
        scene.shade_lights_surface(rays, hits, color, normal, n, rgb, d_weights=weights, d_pixels=pixels, spp=fr.spp,
                                   flags=fl & (binding.MR_MATH_PRODUCT | binding.MR_TRACE_INCOHERENT), d_counts=cnt)
        per_level.append((n, int(cnt.item())))
        if level == depth:
            break
        out = (torch.empty((4 * n, 8), **f32), torch.empty((4 * n, 3), **f32), torch.empty(4 * n, dtype=torch.int32, device="cuda"),
               torch.empty(4 * n, dtype=torch.int32, device="cuda"))
        cnt2 = torch.zeros(1, dtype=torch.int64, device="cuda")
        scene.gen_path_rays_surface(rays, hits, color, normal, weights, pixels, ids, n, out[0], out[1], out[2], out[3], cnt2, spp=fr.spp,
                                    seed=168, bounce=level, kinds=kinds)
        m = int(cnt2.item())
        queues.append((n,) + tuple(o[:m].cpu().numpy() for o in out) + (m,))
        n = m
        rays, weights, pixels, ids = out[0][:n], out[1][:n], out[2][:n], out[3][:n]
    torch.cuda.synchronize()
    return per_level, rgb.cpu().numpy()


def queue_rows(q, ordered):
    t = np.concatenate([q[4].view(np.uint32)[:, None], q[1].view(np.uint32), q[2].view(np.uint32), q[3].view(np.uint32)[:, None]], axis=1)
    return t if ordered else t[np.lexsort(t.T[::-1])]


def check_frame(miro, scene, desc, lights, W, H):
    """(frame with diffuse bounces, frame at depth 0, primary batch) after checking render_specular against the launches by hand"""
    import torch
    from miro_amd import frame
    fr = frame.FrameRenderer(scene, desc, W, H, spp=1)
    fr.generate()
    fr.render_specular(depth=0, lights=lights)
    torch.cuda.synchronize()
    direct = fr.d_rgb.cpu().numpy().copy()
    calls = []
    record_calls(scene, ("gen_path_rays", "gen_path_rays_surface"), calls)
    per_level = fr.render_specular(depth=2, path_tracing=True, path_kinds=ALL_KINDS, lights=lights)
    torch.cuda.synchronize()
    got = fr.d_rgb.cpu().numpy().copy()
    assert [c[0] for c in calls] == ["gen_path_rays_surface"] * 2
    driver_queues = []
    for _, a, _ in calls:                                       # (rays, hits, color, normal, w, pix, ids, n, out_rays, out_w, out_pix, out_ids, cnt)
        m = int(a[12].item())
        driver_queues.append((a[7],) + tuple(o[:m].cpu().numpy() for o in a[8:12]) + (m,))
    for name in ("gen_path_rays", "gen_path_rays_surface"):
        delattr(scene, name)                                    # the wrappers are instance attributes: the class's methods return
    hand_queues = []
    by_hand, want = frame_by_hand(torch, fr, scene, 2, ALL_KINDS, hand_queues)
    print("rays and shadow rays per level %s (by hand %s); brightest pixel %.4g, at depth 0 %.4g" % (per_level, by_hand, got.max(), direct.max()))
    assert per_level == by_hand and len(per_level) == 3 and len(driver_queues) == len(hand_queues) == 2
    single = True                                               # the queue so far was generated chunk by single chunk: its order is fixed
    for dq, hq in zip(driver_queues, hand_queues):
        assert dq[0] == hq[0] and dq[5] == hq[5]
        single = single and dq[0] <= CHUNK
        assert queue_rows(dq, single).tobytes() == queue_rows(hq, single).tobytes()
    scale = float(want.max())
    assert np.isfinite(got).all() and scale > 0
    assert np.allclose(got, want, rtol=1e-5, atol=1e-6 * scale)
    return got, direct, fr


@pytest.mark.gpu
def test_flower_frame_with_diffuse_bounces(miro):
    """flower_scene() at 48 x 32 through render_specular(depth=2, path_tracing=True, all three kinds, lights=...): it no longer
    raises; ray counts per level and the child queues equal those of the same launches made by hand (in order where every queue
    so far came from a single chunk, as sets otherwise), the pixels agree within the bound for float-atomic order; the bounces
    add light."""
    from miro_amd import scenes
    s = miro.Scene(0)
    desc = scenes.flower_setup(s)
    got, direct, _ = check_frame(miro, s, desc, desc["lights"], 48, 32)
    assert (got >= direct - 1e-6 * got.max()).all() and (got > direct).any()


@pytest.mark.gpu
def test_stone_room_frame_lights_the_umbra(miro):
    """The stone room at 32 x 24 likewise; and the floor pixels whose depth-0 frame is exactly 0 -- the umbra under the mirror
    sphere and the floor beside the disc light's beam; the stone floor has ks = kt = 0, so only Ray::random's bounce can reach
    them -- sum to more than 0 at depth 2 (one sample per pixel: a single pixel's bounce may still land in the dark)."""
    from miro_amd import scenes
    desc = scenes.photon_room_stone()
    s = product_textured_room(miro, desc)
    got, direct, fr = check_frame(miro, s, desc, [desc["disc_light"]], 32, 24)
    prim = fr.d_hits.cpu().numpy().view(miro.HIT_DTYPE).reshape(-1)["prim"]
    umbra = (prim != MISS) & ((prim & np.uint32(PLANE_BIT)) != 0) & (direct == 0).all(axis=1)
    print("stone room: %d floor pixels in the umbra, their sum %.4g" % (umbra.sum(), got[umbra].sum()))
    assert umbra.sum() > 0 and got[umbra].sum() > 0 and (got[umbra] >= 0).all()


# ---- 9. routing --------------------------------------------------------------------------------------------------------------
ROUTED = ("hit_surface", "gen_path_rays", "gen_path_rays_surface", "gen_secondary_rays", "trace_device", "trace_level")


@pytest.mark.gpu
def test_checker_room_takes_the_surface_children_on_request(miro):
    """A room whose table holds checkers only: called as before it issues gen_path_rays and no hit_surface; with
    surface_children=True it issues hit_surface and gen_path_rays_surface, floor pixels differ, and the first level's diffuse
    children of floor hits carry mr_texture_lookup's colour at mr_hit_uv's coordinates (w0 = 1) instead of m_diffuse."""
    import torch
    from miro_amd import frame, scenes
    from test_square_surface import checker_room
    s = miro.Scene(0)
    desc = scenes.textured_room_setup(s, checker_room())
    assert s.n_textures == 2 and not s.procedural
    W, H = 24, 16
    fr = frame.FrameRenderer(s, desc, W, H, spp=1)
    fr.generate()
    calls = []
    record_calls(s, ROUTED, calls)
    fr.render_specular(depth=1, path_tracing=True, path_kinds=ALL_KINDS)
    torch.cuda.synchronize()
    before, names_before = fr.d_rgb.cpu().numpy().copy(), [c[0] for c in calls]
    assert names_before == ["trace_device", "gen_path_rays", "trace_device"]
    del calls[:]
    fr.render_specular(depth=1, path_tracing=True, path_kinds=ALL_KINDS, surface_children=True)
    torch.cuda.synchronize()
    after = fr.d_rgb.cpu().numpy().copy()
    assert [c[0] for c in calls] == ["trace_device", "hit_surface", "gen_path_rays_surface", "trace_device"]
    a = calls[2][1]                                             # (rays, hits, color, normal, w, pix, ids, n, out_rays, out_w, out_pix, out_ids, cnt)
    n, m = a[7], int(a[12].item())
    assert n == W * H and a[4] is None and a[6] is None
    hits = a[1].cpu().numpy().view(miro.HIT_DTYPE).reshape(-1)
    floor = np.nonzero((hits["prim"] != MISS) & ((hits["prim"] & np.uint32(PLANE_BIT)) != 0))[0]
    differ = (before != after).any(axis=1)
    print("checker room: %d floor rays, %d children, %d pixels differ (%d of them on the floor)" % (len(floor), m, differ.sum(), differ[floor].sum()))
    assert len(floor) > n // 8 and differ[floor].any() and np.isfinite(after).all()
    uv = torch.empty((n, 2), dtype=torch.float32, device="cuda")
    tex = torch.empty((n, 3), dtype=torch.float32, device="cuda")
    s.hit_uv(a[0], a[1], n, uv)
    s.texture_lookup(1, uv, n, tex)                             # checker_room(): the floor plane's material 5 has texture 1
    torch.cuda.synchronize()
    out_ids, out_w = a[11][:m].cpu().numpy().view(np.uint32), a[9][:m].cpu().numpy()
    want_id = child_id(floor, 3)
    order = np.argsort(out_ids, kind="stable")
    slot = order[np.minimum(np.searchsorted(out_ids[order], want_id), m - 1)]
    assert np.array_equal(out_ids[slot], want_id)
    assert out_w[slot].tobytes() == tex.cpu().numpy()[floor].tobytes()
    assert len(np.unique(out_w[slot], axis=0)) == 2             # the two colours of the checker, not 0.9 x white


@pytest.mark.gpu
def test_untextured_teapot_and_refusals(miro):
    """No texture table: path tracing with MR_PATH_DIFFUSE calls neither surface entry.  surface_children=False with
    MR_PATH_DIFFUSE on the flower: ValueError before any launch; surface_children=True with fused: ValueError."""
    import torch
    from miro_amd import frame, scenes
    desc = scenes.SCENES["teapot"]
    s = miro.Scene(0)
    scenes.populate(s, desc)
    s.build(4)
    fr = frame.FrameRenderer(s, desc, 24, 24, spp=2)
    fr.generate()
    calls = []
    record_calls(s, ROUTED, calls)
    fr.render_specular(depth=1, path_tracing=True, path_kinds=ALL_KINDS)
    torch.cuda.synchronize()
    names = [c[0] for c in calls]
    assert "gen_path_rays" in names and "hit_surface" not in names and "gen_path_rays_surface" not in names
    del calls[:]
    with pytest.raises(ValueError):
        fr.render_specular(depth=1, path_tracing=True, path_kinds=ALL_KINDS, surface_children=True, fused=True)
    assert calls == []
    f = miro.Scene(0)
    fdesc = scenes.flower_setup(f)
    ff = frame.FrameRenderer(f, fdesc, 12, 8, spp=1)
    ff.generate()
    record_calls(f, ROUTED + ("shade_lights_surface", "shade_accumulate_surface", "gen_shadow_rays"), calls)
    with pytest.raises(ValueError):
        ff.render_specular(depth=1, path_tracing=True, path_kinds=ALL_KINDS, lights=fdesc["lights"], surface_children=False)
    assert calls == []
    ff.render_specular(depth=1, path_tracing=True, lights=fdesc["lights"], surface_children=False)   # mirror | refract: still served
    assert "gen_path_rays" in [c[0] for c in calls] and "gen_path_rays_surface" not in [c[0] for c in calls]


# ---- 10. argument errors -----------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_surface_path_argument_errors(miro, room):
    """NULL d_color / d_normal and an address = 2 mod 4: MR_ERR_INVALID, the message names the argument; kinds 0 and 8, and
    out_capacity 0 with n > 0: MR_ERR_INVALID; a host-only scene: MR_ERR_STATE; n = 0: MR_OK and *d_count = 0."""
    import torch
    from test_distribution import host_scene
    L = miro.lib()
    n = 64
    color, normal = room.surface()
    out = (torch.empty((4 * n, 8), dtype=torch.float32, device="cuda"), torch.empty((4 * n, 3), dtype=torch.float32, device="cuda"),
           torch.empty(4 * n, dtype=torch.int32, device="cuda"), torch.empty(4 * n, dtype=torch.int32, device="cuda"))
    cnt = torch.full((1,), 99, dtype=torch.int64, device="cuda")

    def call(scene=room.scene.h, color=color.data_ptr(), normal=normal.data_ptr(), n=n, kinds=ALL_KINDS, capacity=4 * n, spp=1):
        return getattr(L, NAME)(scene, room.rays.data_ptr(), room.hits.data_ptr(), color, normal, None, None, None, n, spp, 168, 0, kinds,
                                out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(), out[3].data_ptr(), cnt.data_ptr(), capacity, None, None)

    assert call(color=None) == -1 and b"d_color" in L.mr_last_error() and NAME.encode() in L.mr_last_error()
    assert call(normal=None) == -1 and b"d_normal" in L.mr_last_error()
    assert call(color=color.data_ptr() + 2) == -1 and b"d_color" in L.mr_last_error() and b"aligned" in L.mr_last_error()
    assert call(normal=normal.data_ptr() + 2) == -1 and b"d_normal" in L.mr_last_error() and b"aligned" in L.mr_last_error()
    assert call(kinds=0) == -1 and call(kinds=8) == -1 and b"kinds" in L.mr_last_error()
    assert call(capacity=0) == -1 and b"out_capacity" in L.mr_last_error() and NAME.encode() in L.mr_last_error()
    assert call(spp=0) == -1
    host = host_scene(miro)
    assert call(scene=host.h) == -5
    torch.cuda.synchronize()
    assert int(cnt.item()) == 99                                # a refused call writes nothing
    assert call(n=0) == 0 and call(n=0, capacity=0) == 0
    torch.cuda.synchronize()
    assert int(cnt.item()) == 0
    assert call(color=color.data_ptr() + 4, normal=normal.data_ptr() + 4, n=n - 1) == 0       # 4-byte aligned is enough
    torch.cuda.synchronize()
    assert 0 < int(cnt.item()) <= 4 * n
