"""mr_trace_photons -- Scene::tracePhotons / traceCausticPhotons (Scene.cpp:351-472) with Scene::tracePhoton (:529-655) on
the device -- against a restatement of tracePhoton written here in numpy float32, wavefront style (all live photons of a
depth at once).  The restatement uses the oracle only for what the oracle is already pinned or tested for: Scene.trace for
the hits, hit_attrs for P / N, path_rays(kinds=4, ids=emission, bounce=depth) for the diffuse continuation, miro_math for
the Fresnel coefficient, orc_hash for the draws (a vectorised pcg32 checked against it).  It imports nothing from the
product; scene descriptions (data) come from miro_amd.scenes.  PARITY UNPINNED: the checker is a restatement written from
the cited lines of the reference.

The keys of the random draws and the termination rule are documented next to mr_trace_photons in include/miro_hip.h."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import kernel_budget  # noqa: E402
F = np.float32
EPS = F(1e-4)                                                   # Miro.h:9
PI = F(3.1415926535897932384626433832795028841972)              # Miro.h:10
MISS, PLANE_BIT = 0xFFFFFFFF, 0x80000000
RECORD = np.dtype([("pos", "<f4", 3), ("dir", "<f4", 3), ("power", "<f4", 3), ("emission", "<u4"), ("depth", "<u4"), ("flags", "<u4")])


# ---- the restatement ---------------------------------------------------------------------------------------------------
def pcg32(x):
    x = np.asarray(x, np.uint32)
    with np.errstate(over="ignore"):
        state = x * np.uint32(747796405) + np.uint32(2891336453)
        word = ((state >> ((state >> np.uint32(28)) + np.uint32(4))) ^ state) * np.uint32(277803737)
    return (word >> np.uint32(22)) ^ word


def unit01(h):
    return (h >> np.uint32(8)).astype(F) * F(1.0 / 16777216.0)


def dot3(a, b):
    return (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]


def cross3(a, b):
    return np.array([a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]], F)


def reflect_dir(d, N):                                          # Ray::reflect, default build (Ray.h:160-162)
    two = 2 * dot3(N, d)
    r = d - two[:, None] * N
    inv = F(1) / np.sqrt((r[:, 0] * r[:, 0] + r[:, 1] * r[:, 1]) + r[:, 2] * r[:, 2])
    return r * inv[:, None]


class Walker:
    """tracePhoton for emissions first ... first + count - 1 of one disc light."""

    def __init__(self, po, scene, materials, prim_mat, plane_mat, light, caustic, seed, max_depth=5):
        self.po, self.scene = po, scene
        self.mats = np.ascontiguousarray(materials, F).reshape(-1, 11)
        self.prim_mat = np.ascontiguousarray(prim_mat, np.uint32)
        self.plane_mat = np.ascontiguousarray(plane_mat, np.uint32)
        self.caustic, self.seed, self.max_depth = bool(caustic), int(seed), int(max_depth)
        self.pos, self.nrm = np.asarray(light["position"], F), np.asarray(light["normal"], F)
        self.radius = F(light["radius"])
        t1 = cross3(np.array([0, 0, 1], F), self.nrm)           # getTangents (Utility.h:25-31)
        if float((t1[0] * t1[0] + t1[1] * t1[1]) + t1[2] * t1[2]) < 1e-6:
            t1 = cross3(np.array([0, 1, 0], F), self.nrm)
        self.t1, self.t2 = t1, cross3(t1, self.nrm)
        k = PI * self.radius * self.radius                      # Scene.cpp:384
        if self.caustic:
            k = k / F(10)                                       # :446
        self.power = (np.asarray(light["color"], F) * F(light["wattage"])) * k
        self.hdir = pcg32(np.uint32(seed))
        self.hevent = pcg32(np.uint32(seed ^ 0x70686f74))
        self.hdisc = pcg32(np.uint32(seed ^ 0x64697363))

    def emit(self, e):
        hd = pcg32(self.hdisc ^ e)
        x, y, done = np.zeros(len(e), F), np.zeros(len(e), F), np.zeros(len(e), bool)
        for a in range(64):                                     # sampleDisc (Utility.h:82-95), attempt a
            with np.errstate(over="ignore"):
                hk = pcg32(hd + np.uint32(a))
            xr = (2 * unit01(pcg32(hk)) - 1) * self.radius
            yr = (2 * unit01(pcg32(hk ^ np.uint32(0x68bc21eb))) - 1) * self.radius
            ok = ~done & ~(xr * xr + yr * yr > self.radius * self.radius)
            x[ok], y[ok] = xr[ok], yr[ok]
            done |= ok
            if done.all():
                break
        return self.pos[None, :] + (x[:, None] * self.t1[None, :] + y[:, None] * self.t2[None, :])

    def walk(self, first, count):
        """Returns (records sorted by emission then depth, stores per emission, segments per emission)."""
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
            P, N = self.scene.hit_attrs(hits, rays)
            N = N * (F(1) / np.sqrt((N[:, 0] * N[:, 0] + N[:, 1] * N[:, 1]) + N[:, 2] * N[:, 2]))[:, None]      # Scene.cpp:262
            prim = hits["prim"]
            is_plane = (prim & np.uint32(PLANE_BIT)) != 0
            mid = np.where(is_plane, self.plane_mat[np.where(is_plane, prim & np.uint32(0x7FFFFFFF), 0)] if len(self.plane_mat) else 0,
                           self.prim_mat[np.where(is_plane, 0, prim)])
            mt = self.mats[mid]
            avg = lambda c: ((c[:, 0] + c[:, 1]) + c[:, 2]) / F(3)      # Vector3::average
            p0 = avg(mt[:, 0:3])
            p1 = p0 + avg(mt[:, 3:6])
            p2 = p1 + avg(mt[:, 6:9])
            with np.errstate(over="ignore"):
                hev = pcg32(self.hevent ^ e) + np.uint32(2 * depth)
                rnd = unit01(pcg32(pcg32(hev)))
                rnd2 = unit01(pcg32(pcg32(hev + np.uint32(1))))
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
            go_diff = diffuse if (depth > 1 or not self.caustic) else np.zeros(len(e), bool)
            no, nd, npw, alive = o.copy(), d.copy(), pw.copy(), np.zeros(len(e), bool)
            ix = np.nonzero(go_diff)[0]
            if len(ix):
                ch, _, _, _, kinds = self.scene.path_rays(self.mats, self.prim_mat, rays[ix], hits[ix], ids=e[ix], seed=self.seed,
                                                          bounce=depth, kinds=4)
                assert len(ch) == len(ix) and (kinds == 3).all()
                cd = np.stack([ch["dx"], ch["dy"], ch["dz"]], axis=1)
                co = np.stack([ch["ox"], ch["oy"], ch["oz"]], axis=1)
                nd[ix] = cd
                no[ix] = co + EPS * cd                          # Ray::random starts at P + eps * d; tracePhoton adds eps * d again
                npw[ix] = (mt[ix, 0:3] * pw[ix]) * (F(1) / p0[ix])[:, None]      # diffuseColor * power / prob[0] (:608)
                alive[ix] = True
            # ---- mirror / transmit (:610-649); a global photon whose first event is specular dies
            if depth == 1 and not self.caustic:
                mirror[:] = False
                transmit[:] = False
            use_reflect = mirror.copy()
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
                rx = ix[~fres]
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


def restate(walker, target, max_emissions, chunk=8192):
    """Scene::tracePhotons' serial loop: emit until `target` photons are stored (the last emission's records all count)."""
    recs, stores, segs = [], [], []
    emitted = 0
    while emitted < max_emissions and sum(int(s.sum()) for s in stores) < target:
        n = min(chunk, max_emissions - emitted)
        r, s, g = walker.walk(emitted, n)
        recs.append(r); stores.append(s); segs.append(g)
        emitted += n
    stores = np.concatenate(stores) if stores else np.zeros(0, np.int64)
    segs = np.concatenate(segs) if segs else np.zeros(0, np.int64)
    recs = np.concatenate(recs) if recs else np.zeros(0, RECORD)
    cum = np.cumsum(stores)
    E = int(np.searchsorted(cum, target, side="left")) + 1 if (target > 0 and len(cum) and cum[-1] >= target) else (0 if target == 0 else emitted)
    recs = recs[recs["emission"] < E]
    return dict(emitted=E, stored=len(recs), segments=int(segs[:E].sum()), records=recs, stores=stores[:E])


def oracle_map(po, res, max_photons):
    m = po.PhotonMap(max_photons)
    r = res["records"]
    if len(r):
        m.store(r["power"], r["pos"], r["dir"])
    if res["emitted"]:
        m.scale_photon_power(float(F(1) / F(res["emitted"])))
    m.balance()
    return m


# ---- scenes --------------------------------------------------------------------------------------------------------------
def material_table(desc):
    return np.array([list(kd) + list(ks) + list(kt) + [sh, ri] for kd, ks, kt, sh, ri in desc["materials"]], F)


def plane_materials(desc):
    return np.array([o[3] if len(o) > 3 else 0 for o in desc["objects"] if o[0] == "plane"], np.uint32)


def oracle_room(po, name):
    from miro_amd import scenes
    desc = scenes.SCENES[name]
    s = po.Scene()
    scenes.populate(s, desc)
    s.build(4)
    return s, desc


def room_walker(po, name, caustic, seed=168, max_depth=5):
    s, desc = oracle_room(po, name)
    return Walker(po, s, material_table(desc), desc["prim_material"], plane_materials(desc), desc["disc_light"], caustic, seed, max_depth), desc


def grey_box(po, rho, lo=(-1.0, -1.0, -1.0), hi=(1.0, 1.0, 1.0)):
    """A closed box of 12 triangles (normals pointing in), one grey Lambert of albedo rho, the disc light inside."""
    (x0, y0, z0), (x1, y1, z1) = lo, hi
    faces = [((x0, y0, z0), (x0, y0, z1), (x0, y1, z1), (x0, y1, z0), (1, 0, 0)), ((x1, y0, z0), (x1, y1, z0), (x1, y1, z1), (x1, y0, z1), (-1, 0, 0)),
             ((x0, y0, z0), (x1, y0, z0), (x1, y0, z1), (x0, y0, z1), (0, 1, 0)), ((x0, y1, z0), (x0, y1, z1), (x1, y1, z1), (x1, y1, z0), (0, -1, 0)),
             ((x0, y0, z0), (x0, y1, z0), (x1, y1, z0), (x1, y0, z0), (0, 0, 1)), ((x0, y0, z1), (x1, y0, z1), (x1, y1, z1), (x0, y1, z1), (0, 0, -1))]
    s = po.Scene()
    for a, b, c, d, n in faces:
        s.add_triangle(a + b + c, n * 3)
        s.add_triangle(a + c + d, n * 3)
    s.build(4)
    mats = np.array([[rho, rho, rho, 0, 0, 0, 0, 0, 0, np.inf, 1.0]], F)
    light = dict(position=(0.1, 0.9, -0.05), normal=(0.0, -1.0, 0.0), color=(1.0, 0.8, 0.6), wattage=50.0, radius=0.5)
    return s, mats, np.zeros(12, np.uint32), light


# ---- without a GPU -------------------------------------------------------------------------------------------------------
def test_pcg32_is_the_oracles_hash(oracle):
    x = np.concatenate([np.arange(64, dtype=np.uint32), np.random.default_rng(1).integers(0, 2 ** 32, 1000, dtype=np.uint64).astype(np.uint32)])
    want = np.array([oracle.lib().orc_hash(int(v)) for v in x], np.uint32)
    assert np.array_equal(pcg32(x), want)


def test_abi_of_the_photon_tracer(miro):
    """The header declares mr_trace_photons, the library exports it, EXPORTED_SYMBOLS matches; struct sizes are the header's;
    the MR_ERR_INVALID cases return -1 with a message before any device call (this runs on a machine without a device)."""
    from miro_amd import binding
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "miro_hip.h")).read(), flags=re.S)
    assert re.search(r"\bmr_trace_photons\s*\(", src)
    L = miro.lib()
    assert hasattr(L, "mr_trace_photons") and "mr_trace_photons" in miro.EXPORTED_SYMBOLS
    assert C.sizeof(binding.DiscLight) == 11 * 4
    assert C.sizeof(binding.PhotonTraceDesc) == 11 * 4 + 6 * 4 + 6 * 4
    assert C.sizeof(binding.PhotonTraceResult) == 32
    assert binding.PHOTON_RECORD_DTYPE.itemsize == 48 == RECORD.itemsize

    s = miro.Scene()
    s.add_triangle([0, 0, 0, 1, 0, 0, 0, 1, 0], [0, 0, 1] * 3)
    s.build(4, host_only=True)
    m = miro.PhotonMap(100)

    def desc(**kw):
        d = binding.PhotonTraceDesc()
        d.light.position[:] = (0, 1, 0)
        d.light.normal[:] = kw.get("normal", (0, -1, 0))
        d.light.color[:] = (1, 1, 1)
        d.light.wattage, d.light.radius = 10.0, kw.get("radius", 0.5)
        d.target, d.max_emissions, d.max_depth = 10, kw.get("max_emissions", 100), kw.get("max_depth", 0)
        return d

    res = binding.PhotonTraceResult()
    ok = desc()
    for args, word in (((None, m.h, C.byref(ok)), b"NULL"), ((s.h, None, C.byref(ok)), b"NULL"), ((s.h, m.h, None), b"NULL"),
                       ((s.h, m.h, C.byref(desc(max_emissions=0))), b"max_emissions"), ((s.h, m.h, C.byref(desc(radius=0.0))), b"radius"),
                       ((s.h, m.h, C.byref(desc(radius=-1.0))), b"radius"), ((s.h, m.h, C.byref(desc(normal=(0, 0, 0)))), b"normal"),
                       ((s.h, m.h, C.byref(desc(max_depth=33))), b"max_depth")):
        assert L.mr_trace_photons(*args, C.byref(res), None, 0, None) == -1
        assert word in L.mr_last_error()
    # a host_only scene: MR_ERR_STATE, never a CPU walk; so is a map that was balanced
    assert L.mr_trace_photons(s.h, m.h, C.byref(ok), C.byref(res), None, 0, None) == -5
    assert b"CPU" in L.mr_last_error()
    t = miro.Scene()
    t.add_triangle([0, 0, 0, 1, 0, 0, 0, 1, 0], [0, 0, 1] * 3)
    assert L.mr_trace_photons(t.h, m.h, C.byref(ok), C.byref(res), None, 0, None) == -5      # not built
    m2 = miro.PhotonMap(100, device=1)
    assert L.mr_trace_photons(s.h, m2.h, C.byref(ok), C.byref(res), None, 0, None) == -1 and b"device" in L.mr_last_error()
    assert m.count() == 0


RHO, N_BOX = 0.6, 20000


def test_restatement_against_the_closed_box_expectation(oracle):
    """The restatement against something that is not itself: in a closed box whose only material is a grey Lambert of albedo
    rho no photon escapes, every hit is diffuse with probability prob[0] = rho, so emission i stores at hit k = 2 ... max_depth + 1
    with probability rho^k: E[s] = rho^2 + ... + rho^(max_depth + 1).  The mean over N emissions must lie within 4 standard errors
    (from the sample itself; about 6e-5 of seeds fail by chance, the seed is fixed).  Every stored power is the emitted power up
    to the rounding of the update kd * power / prob[0] -- six operations per bounce (two additions and a division for prob[0],
    its reciprocal, two products), each within 2^-24 relative."""
    max_depth = 5
    s, mats, pm, light = grey_box(oracle, RHO)
    w = Walker(oracle, s, mats, pm, np.zeros(0, np.uint32), light, caustic=False, seed=2024, max_depth=max_depth)
    recs, stores, segs = w.walk(0, N_BOX)
    rho = float(F(RHO))
    want = sum(rho ** k for k in range(2, max_depth + 2))
    mean, se = stores.mean(), stores.std(ddof=1) / np.sqrt(N_BOX)
    print("stores per emission: mean %.5f, expected %.5f, standard error %.5f" % (mean, want, se))
    assert abs(mean - want) <= 4 * se
    assert len(recs) == stores.sum() and (recs["depth"] >= 2).all() and (recs["depth"] <= max_depth + 1).all()
    assert (recs["flags"] == 0).all()
    assert (segs >= 1).all() and (segs <= max_depth + 1).all() and (stores <= segs - 1).all()
    rel = np.abs(recs["power"].astype(np.float64) / w.power.astype(np.float64)[None, :] - 1).max(axis=1)
    n_ops = 6 * (recs["depth"].astype(np.float64) - 1)
    print("largest power error %.3g (bound %.3g at that depth)" % (rel.max(), (n_ops * 2.0 ** -24)[rel.argmax()]))
    assert (rel <= n_ops * 2.0 ** -24 * 1.001).all()
    # every stored position lies on the box, every incoming direction is a unit vector
    on_wall = (np.abs(np.abs(recs["pos"]) - 1) < 1e-5).any(axis=1)
    assert on_wall.all() and np.allclose(np.linalg.norm(recs["dir"].astype(np.float64), axis=1), 1, atol=1e-5)
    # the termination rule, recomputed from the per-emission counts
    for target in (1, 1000, int(stores.sum()), int(stores.sum()) + 1):
        r = restate(w, target, N_BOX, chunk=N_BOX)
        cum = np.cumsum(stores)
        if cum[-1] >= target:
            E = int(np.argmax(cum >= target)) + 1
            assert r["emitted"] == E and r["stored"] == cum[E - 1] >= target and (E == 1 or cum[E - 2] < target)
        else:
            assert r["emitted"] == N_BOX and r["stored"] == cum[-1]
        assert r["segments"] == segs[:r["emitted"]].sum()


def test_room_scenes_exercise_every_branch(oracle):
    """The room scene description: caustic photons exist (all flagged), global photons never carry the flag, spheres and the
    plane are hit, Fresnel reflection and refraction both occur."""
    w, desc = room_walker(oracle, "photon_room", caustic=True)
    recs, stores, segs = w.walk(0, 4000)
    assert len(recs) > 100 and (recs["flags"] == 1).all() and (recs["depth"] >= 2).all()
    assert (np.abs(recs["pos"][:, 1]) < 1e-4).any()                      # stored on the floor plane
    wg, _ = room_walker(oracle, "photon_room", caustic=False)
    recs, stores, segs = wg.walk(0, 4000)
    assert len(recs) > 1000 and (recs["flags"] == 0).all()


def test_photon_walk_kernels_stay_inside_the_verified_envelope():
    """Every kernel of mr_photon_walk.hip: no dynamic stack; no more spilled VGPRs, no more scratch per lane and no fewer waves
    per SIMD than BOTH its own record (tests/golden/kernel_budget_photon_walk.json, written from the build whose GPU tests were
    green) AND the worst value among the kernels of tests/golden/kernel_budget.json: nothing new ships outside the envelope that
    has run on hardware.  The unit's remarks live in build/mr_photon_walk.remarks.txt, which test_build_budget.py does not read."""
    cur = kernel_budget.unit_kernels("mr_photon_walk")
    assert len(cur) >= 3 and any("photon_walk_kernel" in k for k in cur)
    assert not any("trace_kernel" in k or "frame_kernel" in k for k in cur)
    kernel_budget.assert_inside_envelope(cur, "kernel_budget_photon_walk.json")


# ---- on the MI355X -------------------------------------------------------------------------------------------------------
def product_room(miro, name):
    from miro_amd import scenes
    desc = scenes.SCENES[name]
    s = miro.Scene(0)
    scenes.populate(s, desc)
    s.set_materials(desc["materials"], desc["prim_material"])
    s.build(4)
    return s, desc


def product_trace(miro, scene, desc, target, max_emissions, caustic, max_photons, capacity, light=None, **kw):
    import torch
    m = miro.PhotonMap(max_photons)
    d_rec = torch.full((capacity + 1, 12), -7.0, dtype=torch.float32, device="cuda")       # one sentinel record after the end
    res = scene.trace_photons(m, light or desc["disc_light"], target, max_emissions, caustic=caustic, d_records=d_rec, records_capacity=capacity, **kw)
    torch.cuda.synchronize()
    raw = d_rec.cpu().numpy()
    assert (raw[capacity] == -7.0).all(), "a record was written beyond records_capacity"
    n = min(int(res["stored"]), capacity)
    assert (raw[n:] == -7.0).all()
    return m, res, raw[:n].copy().view(RECORD).reshape(-1)


def same_records(got, want):
    assert len(got) == len(want)
    for f in ("emission", "depth", "flags"):
        assert np.array_equal(got[f], want[f]), f
    for f in ("pos", "dir", "power"):
        bad = np.nonzero((got[f].view(np.uint32) != want[f].view(np.uint32)).any(axis=1))[0]
        assert bad.size == 0, "%s differs at %d of %d records, first %s: %s vs %s" % (f, bad.size, len(got), bad[:3], got[f][bad[:3]], want[f][bad[:3]])


def same_map(miro_map, oracle_map_):
    pa, pla, tpa, pwa = oracle_map_.export()
    pb, plb, tpb, pwb = miro_map.export()
    assert miro_map.count() == oracle_map_.count()
    assert np.array_equal(pa.view(np.uint32), pb.view(np.uint32)) and np.array_equal(tpa, tpb)
    assert np.array_equal(pwa.view(np.uint32), pwb.view(np.uint32))


def check_against_restatement(oracle, miro, name, caustic, target, max_emissions=400000, seed=168):
    scene, desc = product_room(miro, name)
    w, _ = room_walker(oracle, name, caustic, seed=seed)
    want = restate(w, target, max_emissions)
    m, res, recs = product_trace(miro, scene, desc, target, max_emissions, caustic, max_photons=want["stored"] + 10, capacity=want["stored"] + 10, seed=seed)
    print("%s caustic=%d: emitted %d, stored %d, segments %d, rounds %d" % (name, caustic, res["emitted"], res["stored"], res["segments"], res["rounds"]))
    assert (res["emitted"], res["stored"], res["segments"]) == (want["emitted"], want["stored"], want["segments"])
    assert want["stored"] >= target
    same_records(recs, want["records"])
    m.balance(host_only=True)
    same_map(m, oracle_map(oracle, want, want["stored"] + 10))
    return recs


@pytest.mark.gpu
def test_diffuse_room_global_map_is_the_restatements(oracle, miro):
    recs = check_against_restatement(oracle, miro, "photon_room_diffuse", False, 20000)
    assert (recs["flags"] == 0).all() and (recs["depth"] >= 2).all()


@pytest.mark.gpu
@pytest.mark.parametrize("caustic", [1, 0])
def test_room_with_glass_and_mirror_is_the_restatements(oracle, miro, caustic):
    recs = check_against_restatement(oracle, miro, "photon_room", bool(caustic), 6000 if caustic else 20000)
    assert (recs["flags"] == (1 if caustic else 0)).all()


@pytest.mark.gpu
def test_result_does_not_depend_on_the_round_size(miro):
    """round_emissions = 4096, = 100 000 and = 0 give byte-identical maps, records and emitted / stored / segments (`rounds` is
    the one field that describes the launch shape); so do two runs with the same arguments; another seed gives another map."""
    scene, desc = product_room(miro, "photon_room")
    runs = {}
    for key, kw in (("4096", dict(round_emissions=4096)), ("100000", dict(round_emissions=100000)), ("0", {}), ("0 again", {}), ("seed", dict(seed=169))):
        m, res, recs = product_trace(miro, scene, desc, 30000, 1000000, False, 40000, 40000, **kw)
        m.balance(host_only=True)
        runs[key] = ((res["emitted"], res["stored"], res["segments"]), recs.tobytes(), [a.tobytes() for a in m.export()], res["rounds"])
    for key in ("100000", "0", "0 again"):
        assert runs[key][:3] == runs["4096"][:3], key
    assert runs["4096"][3] > runs["100000"][3] >= 1
    assert runs["seed"][1] != runs["0"][1] and runs["seed"][2] != runs["0"][2]


@pytest.mark.gpu
def test_termination(oracle, miro):
    scene, desc = product_room(miro, "photon_room_diffuse")
    # a light that faces away from the scene (above the ceiling, pointing up): nothing is ever stored
    away = dict(desc["disc_light"], position=(0.0, 5.0, 0.0), normal=(0.0, 1.0, 0.0))
    m, res, recs = product_trace(miro, scene, desc, 100, 50000, False, 1000, 1000, light=away)
    assert (res["emitted"], res["stored"]) == (50000, 0) and m.count() == 0 and len(recs) == 0 and res["segments"] == 50000
    # the last emission overshoots the target: its extra records are kept
    w, _ = room_walker(oracle, "photon_room_diffuse", False)
    _, stores, _ = w.walk(0, 4000)
    cum = np.cumsum(stores)
    E = int(np.nonzero((stores >= 2) & (np.arange(len(stores)) > 100))[0][0])          # an emission that stores at least twice
    target = int(cum[E] - stores[E] + 1)
    m, res, recs = product_trace(miro, scene, desc, target, 50000, False, 100000, 100000)
    assert res["emitted"] == E + 1 and res["stored"] == cum[E] > target and m.count() == cum[E]
    assert np.array_equal(np.bincount(recs["emission"], minlength=E + 1), stores[:E + 1])
    # a map smaller than what is stored holds the first max_photons; records_capacity smaller than stored: nothing beyond it
    full_m, full_res, full = product_trace(miro, scene, desc, 5000, 50000, False, 100000, 100000)
    m, res, recs = product_trace(miro, scene, desc, 5000, 50000, False, 1234, 777)
    assert res["stored"] == full_res["stored"] >= 5000 and res["emitted"] == full_res["emitted"]
    assert m.count() == 1234 and len(recs) == 777 and recs.tobytes() == full[:777].tobytes()
    want = oracle.PhotonMap(1234)
    want.store(full["power"], full["pos"], full["dir"])
    want.scale_photon_power(float(F(1) / F(res["emitted"])))
    want.balance()
    m.balance(host_only=True)
    same_map(m, want)
    # target 0: nothing is emitted
    m, res, recs = product_trace(miro, scene, desc, 0, 50000, False, 10, 10)
    assert (res["emitted"], res["stored"], res["segments"]) == (0, 0, 0)
    # a balanced map is immutable
    full_m.balance(host_only=True)
    with pytest.raises(miro.MiroError) as e:
        scene.trace_photons(full_m, desc["disc_light"], 10, 100)
    assert e.value.status == -5


def tied_queries(photon_pos, q, max_dist):
    """Queries for which two photons inside the search radius lie at exactly the same fp32 squared distance (accumulated as
    locate_photons does, PhotonMap.cpp:172-176): a superset of the queries with a tie at rank k or at the first overflow's victim."""
    out = np.zeros(len(q), bool)
    for i in range(len(q)):
        dx = q[i, 0] - photon_pos[:, 0]; dy = q[i, 1] - photon_pos[:, 1]; dz = q[i, 2] - photon_pos[:, 2]
        d2 = (dx * dx + dy * dy) + dz * dz
        d2 = d2[d2 <= F(max_dist) * F(max_dist)]
        out[i] = len(np.unique(d2)) != len(d2)
    return out


K_GATHER, MAX_DIST, W_GATHER = 50, 0.35, 48


def gather_setup(oracle):
    """Restated global + caustic maps of the room and a few thousand surface queries (the primary hits of a small frame)."""
    from helpers import camera_of
    maps = {}
    for caustic, target in ((False, 6000), (True, 2500)):
        w, desc = room_walker(oracle, "photon_room", caustic)
        maps[caustic] = restate(w, target, 400000)
    s, desc = oracle_room(oracle, "photon_room")
    rays = oracle.eye_rays(camera_of(oracle, "photon_room"), W_GATHER, W_GATHER)
    hits = s.trace(rays)
    assert (hits["prim"] != MISS).all()
    P, N = s.hit_attrs(hits, rays)
    N = (N * (F(1) / np.sqrt((N[:, 0] * N[:, 0] + N[:, 1] * N[:, 1]) + N[:, 2] * N[:, 2]))[:, None]).astype(F)
    return maps, P, N


def test_gather_queries_have_few_exact_ties(oracle):
    """The query set of the end-to-end test, with the oracle alone: at most 1 % of the queries have two photons at exactly the
    same squared distance inside the search radius (traced powers are not uniform, so such a tie can change the irradiance)."""
    maps, P, N = gather_setup(oracle)
    for caustic in (False, True):
        tied = tied_queries(maps[caustic]["records"]["pos"], P, MAX_DIST)
        print("caustic=%d: %d photons, %d of %d queries tied" % (caustic, maps[caustic]["stored"], tied.sum(), len(P)))
        assert tied.mean() <= 0.01


@pytest.mark.gpu
def test_traced_maps_answer_queries_like_the_oracles(oracle, miro):
    """End to end: maps traced by the product against oracle maps built from the restatement's records -- `found` and the radius
    of every query equal, the irradiance within test_photon.py's tolerance on the queries without an exact distance tie; and a
    FrameRenderer frame (primary rays + final gather) gathered from the traced maps equals the frame gathered from the same records pushed through store()."""
    import torch
    from miro_amd import frame, scenes
    maps, P, N = gather_setup(oracle)
    scene, desc = product_room(miro, "photon_room")
    traced, stored = {}, {}
    for caustic, target in ((False, 6000), (True, 2500)):
        want = maps[caustic]
        m, res, recs = product_trace(miro, scene, desc, target, 400000, caustic, want["stored"] + 10, want["stored"] + 10)
        same_records(recs, want["records"])
        m.balance()
        ref = oracle_map(oracle, want, want["stored"] + 10)
        wi, wf, wr = ref.irradiance_estimate(P, N, max_dist=MAX_DIST, nphotons=K_GATHER)
        out = torch.empty((len(P), 3), dtype=torch.float32, device="cuda")
        df = torch.empty(len(P), dtype=torch.int32, device="cuda")
        dr = torch.empty(len(P), dtype=torch.float32, device="cuda")
        m.irradiance_estimate(torch.from_numpy(P).cuda(), torch.from_numpy(N).cuda(), len(P), out, max_dist=MAX_DIST, nphotons=K_GATHER, d_found=df, d_r2=dr)
        torch.cuda.synchronize()
        assert np.array_equal(df.cpu().numpy(), wf)
        assert np.array_equal(dr.cpu().numpy().view(np.uint32), wr.view(np.uint32))
        clean = ~tied_queries(want["records"]["pos"], P, MAX_DIST)
        assert clean.mean() >= 0.99 and wf.max() > 0
        got = out.cpu().numpy()
        scale = float(np.abs(wi[clean]).max())
        print("caustic=%d: largest irradiance error %.3g of scale %.3g" % (caustic, np.abs(got[clean] - wi[clean]).max(), scale))
        assert np.abs(got[clean] - wi[clean]).max() <= 2e-5 * scale
        traced[caustic] = m
        s2 = miro.PhotonMap(want["stored"] + 10)
        s2.store(recs["power"], recs["pos"], recs["dir"])
        s2.scale_photon_power(float(F(1) / F(res["emitted"])))
        s2.balance()
        stored[caustic] = s2
    frames = []
    for ms in (traced, stored):
        fr = frame.FrameRenderer(scene, scenes.SCENES["photon_room"], 64, 64)
        fr.generate()
        fr.trace_primary()
        fr.final_gather(ms[False], ms[True], nphotons=K_GATHER, max_dist=MAX_DIST)
        torch.cuda.synchronize()
        frames.append(fr.d_rgb.cpu().numpy().copy())
    assert frames[0].tobytes() == frames[1].tobytes() and frames[0].max() > 0


@pytest.mark.gpu
def test_two_million_emissions_rearm_every_wave(miro):
    """Enough emissions that every resident wave re-arms many times: two runs at different round sizes are byte-identical, and the
    stores per emission meet the closed room's analytic expectation (every wall has prob[0] = 0.6; no full restatement here)."""
    import torch
    scene, desc = product_room(miro, "photon_room_diffuse")
    n = 2000000
    out = []
    for rounds in (0, 300000):
        m = miro.PhotonMap(2 * n)
        d_rec = torch.zeros((2 * n, 12), dtype=torch.float32, device="cuda")
        res = scene.trace_photons(m, desc["disc_light"], 0xFFFFFFFF, n, d_records=d_rec, records_capacity=2 * n, round_emissions=rounds)
        torch.cuda.synchronize()
        out.append((res, d_rec, m.count()))
    (ra, da, ca), (rb, db, cb) = out
    assert (ra["emitted"], ra["stored"], ra["segments"]) == (rb["emitted"], rb["stored"], rb["segments"]) and ra["emitted"] == n
    assert ca == cb == ra["stored"] and torch.equal(da, db)
    recs = da[:ra["stored"]].cpu().numpy().view(RECORD).reshape(-1)
    stores = np.bincount(recs["emission"], minlength=n).astype(np.float64)
    p0 = float((F(0.7) + F(0.6) + F(0.5)) / F(3))
    want = sum(p0 ** k for k in range(2, 7))
    se = stores.std(ddof=1) / np.sqrt(n)
    print("stores per emission: mean %.6f, expected %.6f, standard error %.6f" % (stores.mean(), want, se))
    assert abs(stores.mean() - want) <= 4 * se
    assert (np.diff(recs["emission"].astype(np.int64)) >= 0).all() and (recs["depth"] >= 2).all() and (recs["depth"] <= 6).all()
