"""mr_trace_photons_surface -- the photon walk on textured scenes -- against the restatement of tests/test_photon_walk.py with
three changes (SurfaceWalker below):

  * the colour and the normal of a depth's hits come from mr_hit_surface ON THE DEVICE, run over the restatement's own rays
    and the oracle's hits.  That pass is held by test_procedural.py and test_solid_textures.py; the walk under test must give
    every hit the same bits.
  * prob[0] = average(colour) and the new power (colour * power) * (1 / prob[0]) use that colour (Scene.cpp:545-553, :608);
  * the diffuse child is Ray::random about that normal, restated here in numpy float32 (ray_random): getTangents,
    alignHemisphereToVector on po.miro_math's sin / cos / asin01, the keys of include/miro_hip.h, origin P + eps * dir.  The
    oracle's path_rays cannot serve: it bounces about the geometric normal.

Everything else -- emission, the keys of the draws, the termination rule, mirror / Fresnel / refraction -- is the Walker's.
Records are compared as bytes, so NaNs compare too."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import kernel_budget  # noqa: E402
from test_photon_walk import (EPS, MISS, PI, PLANE_BIT, RECORD, Walker, dot3, material_table, oracle_map, oracle_room,  # noqa: E402
                              pcg32, plane_materials, product_room, product_trace, reflect_dir, restate, same_map, same_records, unit01)

F = np.float32
NONE = 0xFFFFFFFF


# ---- the restatement ---------------------------------------------------------------------------------------------------
def cross_rows(a, b):
    """cross(a, b) of Vector3.h, row by row, every product and difference a float32 operation"""
    return np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2], a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], axis=1).astype(F)


def normalised(N):
    """Vector3::normalize (Scene.cpp:262): *= 1 / length"""
    return (N * (F(1) / np.sqrt(dot3(N, N)))[:, None]).astype(F)


def ray_random(po, N, P, e, depth, hdir):
    """Ray::random (Ray.h:124-140) about N at P for emission e at depth `depth`: phi = asin(sqrt(u1)), theta = 2 PI u2,
    alignHemisphereToVector (Utility.h:34-50) on getTangents (:25-31), Ray(P + epsilon * dir, dir) (Ray.h:86-91).
    Returns (origin, direction)."""
    n = len(e)
    N, P = np.ascontiguousarray(N, F), np.ascontiguousarray(P, F)
    with np.errstate(over="ignore"):
        hray = pcg32(hdir ^ e) + np.uint32(4 * depth)
        hk = pcg32(hray + np.uint32(3))
    u1, u2 = unit01(pcg32(hk)), unit01(pcg32(hk ^ np.uint32(0x68bc21eb)))
    zeros = np.zeros(n, F)
    phi = po.miro_math(np.sqrt(u1), zeros)[:, 2]
    theta = (F(2) * PI) * u2
    mp, mt = po.miro_math(phi, zeros), po.miro_math(theta, zeros)
    c1, c2, c3 = mp[:, 0] * mt[:, 1], mp[:, 0] * mt[:, 0], mp[:, 1]
    ez, ey = np.repeat(np.array([[0, 0, 1]], F), n, axis=0), np.repeat(np.array([[0, 1, 0]], F), n, axis=0)
    t1 = cross_rows(ez, N)
    small = dot3(t1, t1).astype(np.float64) < 1e-6                 # float < double literal
    if small.any():
        t1[small] = cross_rows(ey, N)[small]
    t2 = cross_rows(t1, N)
    d = ((t1 * c1[:, None] + t2 * c2[:, None]) + N * c3[:, None]).astype(F)
    d = (d * (F(1) / np.sqrt(dot3(d, d)))[:, None]).astype(F)
    return (P + d * EPS).astype(F), d


class SurfaceWalker(Walker):
    """Walker with a colour / normal source: surface(rays, hits) -> (colour [n, 3], normal [n, 3]) of the rays that hit.  Also
    counts, for the tests that must know what they exercised: stores per material id, mirror / Fresnel-reflection / refraction
    events, and per material id the diffuse continuations whose normal is / is not the normalised geometric one."""

    def __init__(self, po, scene, surface, *a, **kw):
        super().__init__(po, scene, *a, **kw)
        self.surface = surface
        n = len(self.mats)
        self.stores_by_mat, self.go_by_mat, self.bent_by_mat = np.zeros(n, np.int64), np.zeros(n, np.int64), np.zeros(n, np.int64)
        self.events = dict(mirror=0, fresnel=0, refract=0)

    def walk(self, first, count):
        po = self.po
        e = (np.arange(count, dtype=np.uint64) + first).astype(np.uint32)
        d = np.repeat(self.nrm[None, :], count, axis=0).astype(F)
        o = (self.emit(e) + EPS * d).astype(F)                  # Scene.cpp:535
        pw = np.repeat(self.power[None, :], count, axis=0).astype(F)
        flag = np.zeros(count, np.uint32)
        segments = np.zeros(count, np.uint32)
        recs = []
        for depth in range(1, self.max_depth + 2):              # depth after tracePhoton's increment (:538)
            if len(e) == 0:
                break
            rays = np.zeros(len(e), po.RAY_DTYPE)
            rays["ox"], rays["oy"], rays["oz"], rays["tmin"] = o[:, 0], o[:, 1], o[:, 2], 0.0
            rays["dx"], rays["dy"], rays["dz"], rays["tmax"] = d[:, 0], d[:, 1], d[:, 2], 1e12
            hits = self.scene.trace(rays)
            segments[(e - np.uint32(first)).astype(np.int64)] += 1
            keep = hits["prim"] != MISS
            rays, hits, e, o, d, pw, flag = rays[keep], hits[keep], e[keep], o[keep], d[keep], pw[keep], flag[keep]
            if len(e) == 0:
                break
            P, Ng = self.scene.hit_attrs(hits, rays)
            Ng = normalised(Ng)
            col, N = self.surface(rays, hits)                   # diffuseColor (:545-549) and HitInfo::N as Scene::trace leaves it
            col, N = np.ascontiguousarray(col, F), np.ascontiguousarray(N, F)
            prim = hits["prim"]
            is_plane = (prim & np.uint32(PLANE_BIT)) != 0
            mid = np.where(is_plane, self.plane_mat[np.where(is_plane, prim & np.uint32(0x7FFFFFFF), 0)] if len(self.plane_mat) else 0,
                           self.prim_mat[np.where(is_plane, 0, prim)])
            mt = self.mats[mid]
            avg = lambda c: ((c[:, 0] + c[:, 1]) + c[:, 2]) / F(3)      # Vector3::average
            p0 = avg(col)
            p1 = p0 + avg(mt[:, 3:6])
            p2 = p1 + avg(mt[:, 6:9])
            with np.errstate(over="ignore"):
                hev = pcg32(self.hevent ^ e) + np.uint32(2 * depth)
                rnd = unit01(pcg32(pcg32(hev)))
                rnd2 = unit01(pcg32(pcg32(hev + np.uint32(1))))
            with np.errstate(invalid="ignore"):
                diffuse = ~(rnd > p2) & (rnd < p0)
                spec = ~(rnd > p2) & ~diffuse & (rnd < p2)
                mirror = spec & (rnd < p1)
            transmit = spec & ~mirror
            # ---- diffuse event (:564-609)
            if depth > 1:
                st = np.nonzero(diffuse)[0]
                r = np.zeros(len(st), RECORD)
                r["pos"], r["dir"], r["power"], r["emission"], r["depth"], r["flags"] = P[st], d[st], pw[st], e[st], depth, flag[st]
                recs.append(r)
                self.stores_by_mat += np.bincount(mid[st], minlength=len(self.mats))
            go_diff = diffuse if (depth > 1 or not self.caustic) else np.zeros(len(e), bool)
            no, nd, npw, alive = o.copy(), d.copy(), pw.copy(), np.zeros(len(e), bool)
            ix = np.nonzero(go_diff)[0]
            if len(ix):
                co, cd = ray_random(po, N[ix], P[ix], e[ix], depth, self.hdir)
                nd[ix] = cd
                no[ix] = co + EPS * cd                          # Ray::random starts at P + eps * d; tracePhoton adds eps * d again
                with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
                    npw[ix] = (col[ix] * pw[ix]) * (F(1) / p0[ix])[:, None]      # diffuseColor * power / prob[0] (:608)
                alive[ix] = True
                bent = (N[ix].view(np.uint32) != Ng[ix].view(np.uint32)).any(axis=1)
                self.go_by_mat += np.bincount(mid[ix], minlength=len(self.mats))
                self.bent_by_mat += np.bincount(mid[ix][bent], minlength=len(self.mats))
            # ---- mirror / transmit (:610-649); a global photon whose first event is specular dies
            if depth == 1 and not self.caustic:
                mirror[:] = False
                transmit[:] = False
            use_reflect = mirror.copy()
            self.events["mirror"] += int(mirror.sum())
            ix = np.nonzero(transmit)[0]
            if len(ix):
                dN = dot3(d[ix], N[ix])
                enter = dN < 0
                index = mt[ix, 10]
                n1, n2 = np.where(enter, F(1), index).astype(F), np.where(enter, index, F(1)).astype(F)
                nn = np.where(enter[:, None], N[ix], -N[ix]).astype(F)
                md = -d[ix]
                cosT = dot3(md, nn)                             # getReflectionCoefficient (Ray.h:168-199) on miro_math.h
                assert (cosT >= 0).all()
                inside = cosT <= 1                              # mm_acosf is NaN outside [-1, 1]: Rs NaN, the draw fails, refraction
                ac = po.miro_math(np.where(inside, cosT, F(0)), np.zeros(len(ix), F))[:, 3]
                sinT = po.miro_math(ac, np.zeros(len(ix), F))[:, 0]
                q = (n1 / n2) * sinT
                p = q * q
                with np.errstate(invalid="ignore"):
                    sq = np.sqrt(np.where(p > 1, F(0), F(1) - p)).astype(F)
                    fr = (n1 * cosT - sq) / (n1 * cosT + sq)
                Rs = np.where(p > 1, F(1), fr * fr).astype(F)
                fres = inside & (rnd2[ix] < Rs)                 # :637
                use_reflect[ix[fres]] = True
                self.events["fresnel"] += int(fres.sum())
                rx = ix[~fres]
                self.events["refract"] += len(rx)
                if len(rx):                                     # Ray::refract (Ray.h:202-243), default build
                    n1r, n2r, nnr, dr = n1[~fres], n2[~fres], nn[~fres], d[rx]
                    dn = dot3(dr, nnr)
                    energy = (1 - (n1r.astype(np.float64) * n1r.astype(np.float64)) * (1 - dn.astype(np.float64) * dn.astype(np.float64))
                              / (n2r.astype(np.float64) * n2r.astype(np.float64))).astype(F)
                    tir = energy < 0
                    inv_n2 = F(1) / n2r
                    with np.errstate(invalid="ignore"):
                        se = np.sqrt(np.where(tir, F(0), energy)).astype(F)
                    t = ((dr - nnr * dn[:, None]) * n1r[:, None]) * inv_n2[:, None]
                    rd = (t - nnr * se[:, None]).astype(F)
                    if tir.any():
                        rd[tir] = reflect_dir(dr[tir], N[rx][tir])
                    nd[rx] = rd
                    no[rx] = P[rx] + EPS * rd                   # tracePhoton(hit.P, refr.d, ...) (:647)
                    alive[rx] = True
            ix = np.nonzero(use_reflect)[0]
            if len(ix):
                rd = reflect_dir(d[ix], N[ix])
                nd[ix] = rd
                no[ix] = P[ix] + EPS * rd
                alive[ix] = True
            if depth == 1:
                flag = np.where(mirror | transmit, np.uint32(1), flag).astype(np.uint32)
            e, o, d, pw, flag = e[alive], no[alive].astype(F), nd[alive].astype(F), npw[alive].astype(F), flag[alive]
        recs = np.concatenate(recs) if recs else np.zeros(0, RECORD)
        recs = recs[np.lexsort((recs["depth"], recs["emission"]))]
        stores = np.bincount((recs["emission"] - np.uint32(first)).astype(np.int64), minlength=count).astype(np.int64)
        return recs, stores, segments.astype(np.int64)


def material_source(walker):
    """The plain walk's source: the material's own kd and the geometric normal, normalised"""
    def surface(rays, hits):
        _, N = walker.scene.hit_attrs(hits, rays)
        prim = hits["prim"]
        is_plane = (prim & np.uint32(PLANE_BIT)) != 0
        mid = np.where(is_plane, walker.plane_mat[np.where(is_plane, prim & np.uint32(0x7FFFFFFF), 0)] if len(walker.plane_mat) else 0,
                       walker.prim_mat[np.where(is_plane, 0, prim)])
        return walker.mats[mid][:, 0:3], normalised(N)
    return surface


def device_source(scene):
    """mr_hit_surface of the product scene over the restatement's rays and the oracle's hits"""
    import torch

    def surface(rays, hits):
        n = len(rays)
        d_rays = torch.from_numpy(np.ascontiguousarray(rays).view(F).reshape(n, 8).copy()).cuda()
        d_hits = torch.from_numpy(np.ascontiguousarray(hits).view(F).reshape(n, 4).copy()).cuda()
        color = torch.zeros((n, 3), dtype=torch.float32, device="cuda")
        normal = torch.zeros((n, 3), dtype=torch.float32, device="cuda")
        scene.hit_surface(d_rays, d_hits, n, color, normal)
        torch.cuda.synchronize()
        return color.cpu().numpy(), normal.cpu().numpy()
    return surface


# ---- scenes: the photon_room geometry under the textured tables of miro_amd.scenes ---------------------------------------
def product_textured_room(miro, desc):
    from miro_amd import scenes
    s = miro.Scene(0)
    scenes.textured_room_setup(s, desc)
    return s


def textured_walker(oracle, scene, desc, caustic, seed=168, max_depth=5):
    from miro_amd import scenes
    ref = oracle.Scene()                                        # the geometry alone: materials and textures are tables here
    scenes.populate(ref, desc)
    ref.build(4)
    return SurfaceWalker(oracle, ref, device_source(scene), material_table(desc), desc["prim_material"], plane_materials(desc),
                         desc["disc_light"], caustic, seed, max_depth)


def check_surface_against_restatement(oracle, miro, scene, desc, walker, target, max_emissions, caustic, light=None):
    want = restate(walker, target, max_emissions)
    m, res, recs = product_trace(miro, scene, desc, target, max_emissions, caustic, max_photons=want["stored"] + 10,
                                 capacity=want["stored"] + 10, light=light, seed=walker.seed, surface=True)
    print("caustic=%d: emitted %d, stored %d, segments %d, rounds %d" % (caustic, res["emitted"], res["stored"], res["segments"], res["rounds"]))
    assert (res["emitted"], res["stored"], res["segments"]) == (want["emitted"], want["stored"], want["segments"])
    same_records(recs, want["records"])
    assert recs.tobytes() == want["records"].tobytes()
    m.balance(host_only=True)
    same_map(m, oracle_map(oracle, want, want["stored"] + 10))
    return want


# ---- without a GPU -------------------------------------------------------------------------------------------------------
def test_numpy_ray_random_is_the_oracles_diffuse_child(oracle):
    """ray_random about hit_attrs' normal, normalised, against the oracle's path_rays(kinds=4) on 4096 hits of
    photon_room_diffuse (rays from inside the closed room in seeded directions, so every wall and every tangent case of
    getTangents -- the walls z = +-2 have cross((0, 0, 1), N) = 0 -- occurs): origins and directions bit for bit."""
    ref, desc = oracle_room(oracle, "photon_room_diffuse")
    rng = np.random.default_rng(11)
    n = 4096
    rays = np.zeros(n, oracle.RAY_DTYPE)
    o = np.stack([rng.uniform(-1.5, 1.5, n), rng.uniform(0.0, 3.5, n), rng.uniform(-1.5, 1.5, n)], 1)
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1)[:, None]
    for k, (a, b) in enumerate((("ox", "dx"), ("oy", "dy"), ("oz", "dz"))):
        rays[a], rays[b] = o[:, k], d[:, k]
    rays["tmin"], rays["tmax"] = 0.0, 1e12
    hits = ref.trace(rays)
    assert (hits["prim"] != MISS).all() and len(np.unique(hits["prim"])) == 12
    P, N = ref.hit_attrs(hits, rays)
    N = normalised(N)
    ids = rng.integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)
    mats = material_table(desc)
    for seed, depth in ((168, 1), (7, 4)):
        ch, _, _, _, kinds = ref.path_rays(mats, desc["prim_material"], rays, hits, ids=ids, seed=seed, bounce=depth, kinds=4)
        assert len(ch) == n and (kinds == 3).all()
        co, cd = ray_random(oracle, N, P, ids, depth, pcg32(np.uint32(seed)))
        want_o = np.stack([ch["ox"], ch["oy"], ch["oz"]], axis=1)
        want_d = np.stack([ch["dx"], ch["dy"], ch["dz"]], axis=1)
        assert cd.tobytes() == want_d.tobytes() and co.tobytes() == want_o.tobytes()


def test_surface_walker_with_the_material_source_is_the_walker(oracle):
    """The copy of Walker.walk above, fed the material's kd and the geometric normal, stores the records Walker stores: what the
    GPU tests change is the source alone."""
    from miro_amd import scenes
    for caustic in (False, True):
        ref, desc = oracle_room(oracle, "photon_room")
        args = (material_table(desc), desc["prim_material"], plane_materials(desc), scenes.SCENES["photon_room"]["disc_light"], caustic, 168, 5)
        base = Walker(oracle, ref, *args)
        mine = SurfaceWalker(oracle, ref, None, *args)
        mine.surface = material_source(mine)
        a, b = base.walk(100, 3000), mine.walk(100, 3000)
        assert len(a[0]) > 50 and a[0].tobytes() == b[0].tobytes() and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])
        assert mine.events["mirror"] > 0 and mine.events["fresnel"] > 0 and mine.events["refract"] > 0 and mine.bent_by_mat.sum() == 0


def test_photon_walk_surface_kernels_stay_inside_the_verified_envelope():
    """Every kernel of mr_photon_walk_surface.hip: no dynamic stack; no more spilled VGPRs, no more scratch per lane and no fewer
    waves per SIMD than BOTH its own record (tests/golden/kernel_budget_photon_walk_surface.json, written from the build whose
    GPU run of this file was green) AND the worst value among the kernels of tests/golden/kernel_budget.json."""
    cur = kernel_budget.unit_kernels("mr_photon_walk_surface")
    assert len(cur) == 2 and all("photon_walk_surface_kernel" in k for k in cur)
    kernel_budget.assert_inside_envelope(cur, "kernel_budget_photon_walk_surface.json")


# ---- on the MI355X -------------------------------------------------------------------------------------------------------
def run_both(miro, scene, desc, caustic, **kw):
    out = []
    for surface in (False, True):
        m, res, recs = product_trace(miro, scene, desc, 6000, 20000, caustic, 40000, 40000, surface=surface, **kw)
        m.balance(host_only=True)
        out.append(((res["emitted"], res["stored"], res["segments"], res["rounds"]), recs.tobytes(), [a.tobytes() for a in m.export()]))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("caustic", [0, 1])
def test_plain_scene_is_byte_identical_through_both_entry_points(miro, caustic):
    """photon_room, 20 000 emissions at most with a target of 6000 stores, reached in the middle of a round of 4096 (the room
    stores 0.44 photons per emission, 0.47 in the caustic walk, by the restatement of test_photon_walk.py): records, the result's
    counters and the exported balanced map are byte-identical between mr_trace_photons and mr_trace_photons_surface; and again
    after a texture table (that no material names, so no material's kd changes) has been set and cleared."""
    scene, desc = product_room(miro, "photon_room")
    plain, surf = run_both(miro, scene, desc, bool(caustic), round_emissions=4096)
    assert plain[0][1] >= 6000 and 4096 < plain[0][0] < 20000 and plain[0][0] % 4096 != 0 and plain[0][3] > 1
    assert plain == surf
    scene.set_textures([dict(stone=3.0), dict(petal=((0.0, 1.0, 0.0), 2.0))], [NONE] * len(desc["materials"]))
    with pytest.raises(miro.MiroError):
        scene.trace_photons(miro.PhotonMap(10), desc["disc_light"], 10, 100)
    scene.set_textures([])
    plain2, surf2 = run_both(miro, scene, desc, bool(caustic), round_emissions=4096)
    assert plain2 == plain and surf2 == plain


N_MIXED = 30000


@pytest.mark.gpu
@pytest.mark.parametrize("caustic", [0, 1])
def test_mixed_room_is_the_restatements(oracle, miro, caustic):
    """The room with PETAL, LEAF, FLOWER_CENTER, STEM (with texture coordinates) and plain walls, a CHECKER floor plane and the
    plain glass and mirror spheres; N_MIXED emissions, all walked (the target is out of reach).  emitted, stored, segments, the
    records and the balanced map are the restatement's.  The restatement's own events say what was exercised: in the global map
    every texture kind present took at least 50 stores, and mirror, Fresnel reflection and refraction each occur in both maps.
    The restatement's counts at N_MIXED = 30 000 (petal, leaf, flower centre, stem, plain, checker): global 6662 stores --
    1633, 675, 614, 861, 1804, 1075 -- with 2116 mirror, 510 Fresnel-reflection and 4742 refraction events; caustic 7181 stores
    -- 1204, 263, 920, 303, 828, 3663 -- with 6421, 2388 and 21 999.  30 000 emissions suffice."""
    from miro_amd import scenes
    desc = scenes.photon_room_mixed()
    scene = product_textured_room(miro, desc)
    w = textured_walker(oracle, scene, desc, bool(caustic))
    want = check_surface_against_restatement(oracle, miro, scene, desc, w, 0xFFFFFFFF, N_MIXED, bool(caustic))
    print("stores per material %s, events %s, continuations %s" % (w.stores_by_mat.tolist(), w.events, w.go_by_mat.tolist()))
    assert want["emitted"] == N_MIXED and want["stored"] > 1000
    assert w.events["mirror"] > 0 and w.events["fresnel"] > 0 and w.events["refract"] > 0
    if not caustic:
        for mid in (0, 1, 2, 3, 4, 5):                          # petal, leaf, flower centre, stem, plain, checker
            assert w.stores_by_mat[mid] >= 50, mid
    assert w.bent_by_mat.sum() == 0                             # no stone here: every normal is the geometric one


@pytest.mark.gpu
def test_stone_room_is_the_restatements(oracle, miro):
    """The floor plane a STONE of scale 3, two walls STONE of scale 20 with texture coordinates, ks = kt = 0: the map and the
    records are the restatement's, whose diffuse bounces leave along Ray::random about the BUMPED normal.  On at least 90 % of
    the stone hits that continue the surface pass's normal differs from the normalised geometric one (hit_attrs'): the bump is
    exercised.  (The stone walls are x = -2 and z = -2, whose inward normals have a positive largest component, wound so that
    toUVCoordinates is defined on them: on the other walls the reference's own rules leave N un-bumped, or (u, v) NaN -- see
    scenes.photon_room_stone.)"""
    from miro_amd import scenes
    desc = scenes.photon_room_stone()
    scene = product_textured_room(miro, desc)
    w = textured_walker(oracle, scene, desc, False)
    want = check_surface_against_restatement(oracle, miro, scene, desc, w, 8000, 100000, False)
    go, bent = w.go_by_mat[:2].sum(), w.bent_by_mat[:2].sum()
    print("stone continuations %d, bumped %d (per material: continuations %s, bumped %s); stores per material %s" % (
        go, bent, w.go_by_mat.tolist(), w.bent_by_mat.tolist(), w.stores_by_mat.tolist()))
    assert want["stored"] >= 8000 and go > 2000 and bent >= 0.9 * go
    assert w.stores_by_mat[0] >= 50 and w.stores_by_mat[1] >= 50 and w.bent_by_mat[2:].sum() == 0


@pytest.mark.gpu
def test_stone_room_does_not_depend_on_the_round_size(miro):
    """2^19 emissions of max_depth 1 with a target out of reach, in one round of 2^19 -- more emissions than a resident grid has
    lanes, so lanes re-arm with the noise tables staged -- and in rounds of 16 384: d_records and the counters are identical."""
    import torch
    from miro_amd import scenes
    desc = scenes.photon_room_stone()
    scene = product_textured_room(miro, desc)
    n = 1 << 19
    out = []
    for rounds in (n, 16384):
        m = miro.PhotonMap(n)
        d_rec = torch.zeros((n, 12), dtype=torch.float32, device="cuda")
        res = scene.trace_photons(m, desc["disc_light"], 0xFFFFFFFF, n, max_depth=1, d_records=d_rec, records_capacity=n, round_emissions=rounds,
                                  surface=True)
        torch.cuda.synchronize()
        out.append((res, d_rec, m.count()))
    (ra, da, ca), (rb, db, cb) = out
    assert (ra["emitted"], ra["stored"], ra["segments"]) == (rb["emitted"], rb["stored"], rb["segments"]) and ra["emitted"] == n
    assert ra["rounds"] == 1 and rb["rounds"] == n // 16384
    assert ca == cb == ra["stored"] > 10000 and torch.equal(da.view(torch.int32), db.view(torch.int32))


@pytest.mark.gpu
def test_flower_scene_is_the_restatements(oracle, miro):
    """scenes.flower_scene() under its disc light of radius 7 at (50, 50, 40), global map: the records are the restatement's.
    The emission count follows from the restatement alone: it emits (in chunks of 8192) until it has stored 200 records, which
    takes 29 690 emissions (most photons of the radius-7 disc pass the flower; 34 847 segments in all)."""
    from miro_amd import scenes
    scene = miro.Scene(0)
    desc = scenes.flower_setup(scene)
    ref = oracle.Scene()
    scenes.populate(ref, desc)
    ref.build(4)
    light = desc["lights"][0]
    w = SurfaceWalker(oracle, ref, device_source(scene), material_table(desc), desc["prim_material"], np.zeros(0, np.uint32), light, False, 168, 5)
    want = check_surface_against_restatement(oracle, miro, scene, desc, w, 200, 400000, False, light=light)
    print("flower: %d emissions for %d records; stores per material %s" % (want["emitted"], want["stored"], w.stores_by_mat.tolist()))
    assert want["stored"] >= 200


@pytest.mark.gpu
def test_errors_and_routing(miro):
    """NULL arguments, a non-zero reserved word and a balanced map: as the plain call.  mr_trace_photons on the mixed room still
    returns MR_ERR_STATE, naming textures and the new call.  The binding's surface=True reaches the new symbol."""
    from miro_amd import binding, scenes
    L = miro.lib()
    assert hasattr(L, "mr_trace_photons_surface") and "mr_trace_photons_surface" in binding.SURFACE_SYMBOLS
    header = open(os.path.join(ROOT, "include", "miro_hip_surface.h")).read()
    assert "mr_trace_photons_surface(" in header and '#include "miro_hip_surface.h"' in open(os.path.join(ROOT, "include", "miro_hip.h")).read()
    desc = scenes.photon_room_mixed()
    scene = product_textured_room(miro, desc)
    m = miro.PhotonMap(1000)
    d = binding.PhotonTraceDesc()
    d.light.position[:], d.light.normal[:], d.light.color[:] = (0, 3.9, 0), (0, -1, 0), (1, 1, 1)
    d.light.wattage, d.light.radius, d.target, d.max_emissions, d.seed = 100.0, 0.8, 10, 1000, 168      # trace_photons' default seed
    res = binding.PhotonTraceResult()
    for args in ((None, m.h, C.byref(d)), (scene.h, None, C.byref(d)), (scene.h, m.h, None)):
        assert L.mr_trace_photons_surface(*args, C.byref(res), None, 0, None) == -1 and b"NULL" in L.mr_last_error()
    d.reserved[2] = 1
    assert L.mr_trace_photons_surface(scene.h, m.h, C.byref(d), C.byref(res), None, 0, None) == -1 and b"reserved" in L.mr_last_error()
    d.reserved[2] = 0
    assert L.mr_trace_photons(scene.h, m.h, C.byref(d), C.byref(res), None, 0, None) == -5
    assert b"textures" in L.mr_last_error() and b"mr_trace_photons_surface" in L.mr_last_error()
    assert m.count() == 0
    assert L.mr_trace_photons_surface(scene.h, m.h, C.byref(d), C.byref(res), None, 0, None) == 0 and res.stored >= 10 and m.count() == res.stored
    with pytest.raises(miro.MiroError) as e:
        scene.trace_photons(m, desc["disc_light"], 10, 1000)
    assert e.value.status == -5 and "textures" in str(e.value)
    r = scene.trace_photons(miro.PhotonMap(1000), desc["disc_light"], 10, 1000, surface=True)
    assert (r["emitted"], r["stored"]) == (res.emitted, res.stored)
    m.balance(host_only=True)
    with pytest.raises(miro.MiroError) as e:
        scene.trace_photons(m, desc["disc_light"], 10, 1000, surface=True)
    assert e.value.status == -5
