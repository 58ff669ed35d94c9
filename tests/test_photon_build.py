"""mr_photon_map_build_device and mr_trace_photons_resident: the photon map stored, balanced and boxed on the device.

The yardstick everywhere is the library's own HOST path on the same records -- mr_photon_map_store, mr_photon_map_scale,
mr_photon_map_balance -- which this feature leaves as it was.  A device-built map must be indistinguishable from it: the four
arrays of export() (which, on such a map, reads the device arrays back) are compared with np.array_equal on their integer
views, and count().  On tie-free inputs the oracle's PhotonMap is compared as well, as tests/test_photon.py's
test_balance_identical compares it (plane on the nodes that descend).  On tied inputs only the host path is the yardstick:
with a tied median neither it nor the oracle gives the reference's tree (tests/test_photon_reference.py pins both builders to
the reference's own PhotonMap.cpp on maps without one, and measures the rest).  No test asserts a speed."""
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import kernel_budget  # noqa: E402
from helpers import oracle_scene  # noqa: E402
from miro_amd import scenes  # noqa: E402
from test_photon_walk import K_GATHER, MAX_DIST, W_GATHER, product_room, product_trace  # noqa: E402
from test_photon_walk_surface import product_textured_room  # noqa: E402

F = np.float32
INVALID, STATE = -1, -5


def records_of(power, pos, direction):
    """mr_photon_record rows; the fields the build ignores (emission, depth, flags) hold rubbish"""
    rec = np.empty((len(pos), 12), F)
    rec[:, 0:3], rec[:, 3:6], rec[:, 6:9] = pos, direction, power
    rec[:, 9:12] = np.arange(3 * len(pos), dtype=np.uint32).reshape(-1, 3).view(F)
    return rec


def host_map(miro, power, pos, direction, scale, max_photons=None, host_only=True):
    m = miro.PhotonMap(max_photons if max_photons is not None else len(pos) + 10)
    m.store(power, pos, direction)
    m.scale_photon_power(scale)
    m.balance(host_only=host_only)
    return m


def device_map(miro, power, pos, direction, scale, max_photons=None):
    import torch
    m = miro.PhotonMap(max_photons if max_photons is not None else len(pos) + 10)
    rec = torch.from_numpy(records_of(power, pos, direction)).cuda()
    res = m.build_device(rec, len(pos), scale)
    torch.cuda.synchronize()
    return m, res


def same_export(got, want):
    assert got.count() == want.count()
    (pa, pla, tpa, pwa), (pb, plb, tpb, pwb) = got.export(), want.export()
    assert np.array_equal(pa.view(np.uint32), pb.view(np.uint32)), "pos"
    assert np.array_equal(pla, plb), "plane"
    assert np.array_equal(tpa, tpb), "theta_phi"
    assert np.array_equal(pwa.view(np.uint32), pwb.view(np.uint32)), "power"


def unit_rows(rng, n):
    d = rng.randn(n, 3)
    return (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(F)


# ---- without a GPU -------------------------------------------------------------------------------------------------------
def test_symbols_and_prototypes(miro):
    from miro_amd import binding
    L = miro.lib()
    strip = lambda p: re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", p)).read(), flags=re.S)
    for name in ("mr_photon_map_build_device", "mr_trace_photons_resident"):
        assert hasattr(L, name) and name in binding.SURFACE_SYMBOLS and name not in binding.EXPORTED_SYMBOLS
        assert re.search(r"\bmr_status\s+%s\s*\(" % name, strip("miro_hip_surface.h"))
        assert not re.search(r"\b%s\s*\(" % name, strip("miro_hip.h"))
        assert name in open(os.path.join(ROOT, "include", "miro_hip.h")).read()          # the pointer next to the host calls
    assert len(binding.EXPORTED_SYMBOLS) == 69
    assert "mr_photon_build_result" in strip("miro_hip_surface.h")


def test_argument_errors_before_any_device_call(miro):
    """NULL map, NULL or misaligned records, n above 2^24: MR_ERR_INVALID with a message naming the cause, on a machine
    without a device"""
    L = miro.lib()
    m = miro.PhotonMap(100)
    A = 4096                                                    # an aligned, non-NULL address that is never dereferenced
    res = miro.binding.PhotonBuildResult()
    assert L.mr_photon_map_build_device(None, A, 8, 1.0, res, None) == INVALID and b"NULL" in L.mr_last_error()
    assert L.mr_photon_map_build_device(m.h, None, 8, 1.0, res, None) == INVALID and b"NULL" in L.mr_last_error()
    assert L.mr_photon_map_build_device(m.h, A + 2, 8, 1.0, res, None) == INVALID and b"aligned" in L.mr_last_error()
    assert L.mr_photon_map_build_device(m.h, A, (1 << 24) + 1, 1.0, None, None) == INVALID
    assert b"2^24" in L.mr_last_error() and b"mr_photon_map_store" in L.mr_last_error()         # names the host path
    x = np.ones((3, 3), F)
    m.store(x, x, x / np.sqrt(3))
    assert L.mr_photon_map_build_device(m.h, A, 8, 1.0, res, None) == STATE and b"already holds" in L.mr_last_error()
    m.balance(host_only=True)
    assert L.mr_photon_map_build_device(m.h, A, 8, 1.0, res, None) == STATE
    desc = miro.binding.PhotonTraceDesc()
    assert L.mr_trace_photons_resident(None, m.h, desc, 2, None, None, None, 0, None) == INVALID and b"surface" in L.mr_last_error()
    assert L.mr_trace_photons_resident(None, m.h, desc, 0, None, None, None, 0, None) == INVALID and b"NULL" in L.mr_last_error()


def test_photon_build_kernels_stay_inside_the_verified_envelope():
    """Every kernel of mr_photon_build.hip: no scratch, no spills, no dynamic stack, and no fewer waves per SIMD than its own
    record (tests/golden/kernel_budget_photon_build.json, written from the build whose GPU run of this file was green) and
    than the worst kernel of tests/golden/kernel_budget.json."""
    cur = kernel_budget.unit_kernels("mr_photon_build")
    for part in ("build_store_kernel", "radix_scatter_kernel", "build_node_kernel", "build_scatter_kernel", "build_pack_kernel", "build_boxes_kernel"):
        assert any(part in k for k in cur), part
    for name, c in cur.items():
        assert c["scratch_bytes_per_lane"] == 0 and c["vgprs_spilled"] == 0 and c["sgprs_spilled"] == 0, (name, c)
    kernel_budget.assert_inside_envelope(cur, "kernel_budget_photon_build.json")


# ---- on the MI355X -------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("n", [0, 1, 2, 3, 4, 5, 6, 7, 8, 63, 64, 65, 127, 1000, 4095, 4096, 4097, 50000])
def test_sizes(oracle, miro, n):
    """Every arm of the left-balanced median, single-element children, the block-root boundaries at 64 and 4096, more than one
    workgroup per scan and per radix pass.  synthetic_photons on the teapot, scale = 1 / n; against the host path, and for
    n >= 1 against the oracle too (test_balance_identical starts there)."""
    s = oracle_scene(oracle, "teapot")
    v, _, vi, _ = s.arrays()
    pw, pos, d = scenes.synthetic_photons(v, vi, n, 168) if n else (np.zeros((0, 3), F),) * 3
    scale = 1.0 / n if n else 1.0
    got, res = device_map(miro, pw, pos, d, scale)
    assert (res["stored"], res["dropped"]) == (n, 0) and res["deferred"] <= n
    same_export(got, host_map(miro, pw, pos, d, scale))
    if n:
        ref = oracle.PhotonMap(n + 10)
        ref.store(pw, pos, d)
        ref.scale_photon_power(scale)
        ref.balance()
        (pa, pla, tpa, pwa), (pb, plb, tpb, pwb) = ref.export(), got.export()
        assert np.array_equal(pa.view(np.uint32), pb.view(np.uint32)) and np.array_equal(tpa, tpb)
        assert np.array_equal(pwa.view(np.uint32), pwb.view(np.uint32))
        inner = np.arange(n) + 1 < n // 2 - 1
        assert np.array_equal(pla[inner], plb[inner])


def tied_inputs(kind):
    rng = np.random.RandomState(7)
    if kind == "plane":                                          # all on y = 0, half of the zeros written as -0.0f
        n = 5000
        pos = rng.rand(n, 3).astype(F)
        pos[:, 1] = np.where(rng.rand(n) < 0.5, F(-0.0), F(0.0))
        assert np.signbit(pos[:, 1]).sum() > 2000 and (~np.signbit(pos[:, 1])).sum() > 2000
    elif kind == "point":                                        # pure index order, axis 2 throughout
        n = 1000
        pos = np.tile(np.array([[0.25, -1.5, 3.0]], F), (n, 1))
    elif kind == "lattice":                                      # 17 x 241: repeated coordinates on two axes
        n = 17 * 241
        i = rng.permutation(n)
        pos = np.stack([(i % 17) * 0.5, (i // 17) * 0.125, rng.rand(n)], axis=1).astype(F)
    else:                                                        # x takes four values
        n = 3000
        pos = rng.rand(n, 3).astype(F)
        pos[:, 0] = np.array([-1.0, 0.0, 0.5, 2.0], F)[rng.randint(0, 4, n)]
    return rng.rand(n, 3).astype(F), pos, unit_rows(rng, n)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["plane", "point", "lattice", "four_x"])
def test_ties(miro, kind):
    pw, pos, d = tied_inputs(kind)
    got, _ = device_map(miro, pw, pos, d, 0.5)
    want = host_map(miro, pw, pos, d, 0.5)
    same_export(got, want)
    if kind == "point":
        assert (want.export()[1][: len(pos) // 2 - 2] == 2).all()


def special_directions():
    a = F(np.sqrt(0.4))
    up, down = np.nextafter(F(1), F(2)), np.nextafter(F(-1), F(-2))
    return np.array([(0, 0, 1), (0, 0, -1), (1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0),
                     (a, a, 0.4), (-a, a, 0.4), (-a, -a, 0.4), (a, -a, 0.4), (0.5, 0.5, -0.7), (-0.25, -0.25, 0.9),
                     (0, 0, up), (0, 0, down), (0.1, 0.2, up), (0, 0, 0)], F)


@pytest.mark.gpu
def test_direction_bytes(miro):
    """2^20 random unit directions and the specials: theta_phi is the host's for every photon (same_export); every special is
    deferred, and of the random ones at most 1e-4 (the expected share is about 4e-6)."""
    rng = np.random.RandomState(11)
    sp = special_directions()
    n_random = 1 << 20
    d = np.concatenate([sp, unit_rows(rng, n_random)])
    d = d[rng.permutation(len(d))]
    pos, pw = rng.rand(len(d), 3).astype(F), rng.rand(len(d), 3).astype(F)
    got, res = device_map(miro, pw, pos, d, 0.25)
    print("deferred %d of %d (%d specials)" % (res["deferred"], len(d), len(sp)))
    same_export(got, host_map(miro, pw, pos, d, 0.25))
    assert len(sp) <= res["deferred"] <= len(sp) + 1e-4 * n_random


@pytest.mark.gpu
def test_every_photon_deferred(miro):
    rng = np.random.RandomState(12)
    d = special_directions()
    pos, pw = rng.rand(len(d), 3).astype(F), rng.rand(len(d), 3).astype(F)
    got, res = device_map(miro, pw, pos, d, 2.0)
    assert res["deferred"] == len(d) == res["stored"]
    same_export(got, host_map(miro, pw, pos, d, 2.0))


@pytest.mark.gpu
def test_capping_and_state(miro):
    import torch
    rng = np.random.RandomState(13)
    pos, pw, d = rng.rand(8, 3).astype(F), rng.rand(8, 3).astype(F), unit_rows(rng, 8)
    got, res = device_map(miro, pw, pos, d, 0.125, max_photons=5)
    assert (res["stored"], res["dropped"]) == (5, 3)
    same_export(got, host_map(miro, pw, pos, d, 0.125, max_photons=5))
    rec = torch.from_numpy(records_of(pw, pos, d)).cuda()
    for call in (lambda: got.build_device(rec, 8, 1.0), lambda: got.store(pw, pos, d), lambda: got.scale_photon_power(2.0)):
        with pytest.raises(miro.MiroError) as e:
            call()
        assert e.value.status == STATE
    same_export(got, host_map(miro, pw, pos, d, 0.125, max_photons=5))
    # a NaN position is refused and the map stays empty and usable
    bad = pos.copy()
    bad[3, 1] = np.nan
    m = miro.PhotonMap(100)
    with pytest.raises(miro.MiroError) as e:
        m.build_device(torch.from_numpy(records_of(pw, bad, d)).cuda(), 8, 1.0)
    assert e.value.status == INVALID and "finite" in str(e.value) and m.count() == 0
    assert m.build_device(rec, 8, 0.5)["stored"] == 8
    same_export(m, host_map(miro, pw, pos, d, 0.5))
    # every position beyond 1e8: the initial box is not a bound of the photons (Photon_map's constructor), on both paths
    far = (pos * F(1e9) + F(2e8)).astype(F)
    far[:, 1] = -far[:, 1]
    got, _ = device_map(miro, pw, far, d, 1.0)
    same_export(got, host_map(miro, pw, far, d, 1.0))


@pytest.fixture(scope="module")
def sponza_maps(oracle, miro):
    """20 000 synthetic photons on the sponza stand-in through both paths, and 3 000 surface queries, as
    test_irradiance_estimate_matches_oracle makes them"""
    import torch
    s = oracle_scene(oracle, "sponza")
    v, _, vi, _ = s.arrays()
    n = 20000
    pw, pos, d = scenes.synthetic_photons(v, vi, n, 168)
    host = host_map(miro, pw, pos, d, 1.0 / n, host_only=False)
    dev, _ = device_map(miro, pw, pos, d, 1.0 / n)
    _, qpos, qdir = scenes.synthetic_photons(v, vi, 3000, seed=99)
    return host, dev, torch.from_numpy(qpos).cuda(), torch.from_numpy(-qdir).cuda()


@pytest.mark.gpu
@pytest.mark.parametrize("k,md", [(50, 1e10), (4, 1e10), (9, 0.8)])
def test_estimates_equal_the_host_built_maps(miro, sponza_maps, k, md):
    """found and r2 equal, irradiance within 1e-5 of the largest expected value (tests/test_photon.py's figure for summation
    order); small k with a bounded radius is what reads the block boxes"""
    import torch
    host, dev, dq, dn = sponza_maps
    same_export(dev, host)
    out = []
    for m in (host, dev):
        irr = torch.empty((len(dq), 3), dtype=torch.float32, device="cuda")
        found = torch.empty(len(dq), dtype=torch.int32, device="cuda")
        r2 = torch.empty(len(dq), dtype=torch.float32, device="cuda")
        m.irradiance_estimate(dq, dn, len(dq), irr, max_dist=md, nphotons=k, d_found=found, d_r2=r2)
        torch.cuda.synchronize()
        out.append((irr.cpu().numpy(), found.cpu().numpy(), r2.cpu().numpy()))
    (want, wf, wr), (got, gf, gr) = out
    assert np.array_equal(gf, wf) and np.array_equal(gr.view(np.uint32), wr.view(np.uint32))
    assert want.max() > 0 and np.abs(got - want).max() <= 1e-5 * np.abs(want).max()


def stone_room(miro):
    desc = scenes.photon_room_stone()
    return product_textured_room(miro, desc), desc


RESIDENT_CASES = {   # scene, caustic, target, max_emissions, surface, round_emissions: the targets of tests/test_photon_walk*.py
    "diffuse_room": ("photon_room_diffuse", False, 20000, 400000, False, 0),
    "room_global": ("photon_room", False, 20000, 400000, False, 0),
    "room_caustic": ("photon_room", True, 6000, 400000, False, 0),
    "room_global_rounds": ("photon_room", False, 20000, 400000, False, 4096),
    "stone_room": (None, False, 8000, 100000, True, 0),
}


@pytest.mark.gpu
@pytest.mark.parametrize("case", sorted(RESIDENT_CASES))
def test_trace_photons_resident(miro, case):
    """result, d_records and the exported map equal mr_trace_photons / _surface + balance with the same desc; the timing reports
    no read-back and no host store; the host call on the same scene afterwards still gives its old bytes"""
    import torch
    name, caustic, target, max_emissions, surface, rounds = RESIDENT_CASES[case]
    scene, desc = stone_room(miro) if name is None else product_room(miro, name)
    cap = target + 64
    kw = dict(surface=surface, round_emissions=rounds)

    def host():
        m, res, recs = product_trace(miro, scene, desc, target, max_emissions, caustic, cap, cap, **kw)
        m.balance(host_only=True)
        return m, res, recs
    m0, res0, recs0 = host()
    m1, res1, recs1 = product_trace(miro, scene, desc, target, max_emissions, caustic, cap, cap, resident=True, **kw)
    m2, res2, recs2 = host()
    fields = ("emitted", "stored", "segments", "rounds")
    assert [res1[f] for f in fields] == [res0[f] for f in fields] and res0["stored"] >= target
    assert rounds == 0 or res1["rounds"] > 1
    assert recs1.tobytes() == recs0.tobytes()
    assert res1["readback_ms"] == 0 and res1["store_ms"] == 0 and res1["kernel_ms"] > 0 and res0["store_ms"] > 0
    build = res1["build"]
    assert (build["stored"], build["dropped"]) == (res0["stored"], 0) and build["balance_ms"] > 0
    same_export(m1, m0)
    with pytest.raises(miro.MiroError) as e:                     # one map per call
        scene.trace_photons(m1, desc["disc_light"], target, max_emissions, caustic=caustic, resident=True, **kw)
    assert e.value.status == STATE
    assert [res2[f] for f in fields] == [res0[f] for f in fields] and recs2.tobytes() == recs0.tobytes()
    same_export(m2, m0)


@pytest.mark.gpu
def test_through_the_recursion(miro):
    """One 48 x 48, depth-2 render_specular(photon_maps=Scene.photon_maps(...)) frame of the photon room against the same frame
    from host-built maps: within 2e-5 of the largest pixel value, tests/test_gather_level.py's figure for float-atomic order"""
    import torch
    from miro_amd import frame
    scene, desc = product_room(miro, "photon_room")
    target, max_emissions = 6000, 400000
    host = []
    for caustic in (False, True):
        m = miro.PhotonMap(target + 32)
        scene.trace_photons(m, desc["disc_light"], target, max_emissions, caustic=caustic)
        m.balance()
        host.append(m)
    dev = scene.photon_maps(desc["disc_light"], target, max_emissions)
    for a, b in zip(dev, host):
        same_export(a, b)
    fr = frame.FrameRenderer(scene, desc, W_GATHER, W_GATHER)
    fr.generate()
    frames = []
    for maps in (host, dev):
        fr.render_specular(depth=2, photon_maps=tuple(maps), nphotons=K_GATHER, max_dist=MAX_DIST)
        torch.cuda.synchronize()
        frames.append(fr.d_rgb.cpu().numpy().astype(np.float64))
    assert frames[0].max() > 0 and np.abs(frames[1] - frames[0]).max() <= 2e-5 * frames[0].max()
