"""The photon map against the reference's own PhotonMap.cpp.

tests/golden/photon_ref/*.npz is what oracle/_ref/photon_ref computed: the reference's Photon_map, compiled unchanged and driven
by oracle/ref_photon_driver.cpp (tests/golden/make_photon_ref.py writes the fixtures and is imported here for the seeded inputs;
the fixtures hold the inputs' sha256 only).  A map has a TIED MEDIAN if some node with a child has another photon in its subtree
with the same pos[plane].

PINNED, exactly: on the maps without a tied median the oracle (tree, found, dist2[0] and the irradiance bit for bit, on every
query), the product's host balance and device build (tree) and mr_irradiance_estimate (found and dist2[0] on every query; the
irradiance to summation order against the reference's own candidate set) are the reference's.
NOT PINNED: maps with a tied median, where product and oracle select the median by (coordinate, index) and the reference's
median_split does not -- three such maps carry a strict xfail and the measured deviation is in DESIGN.md "Oracle"; and which of
two photons at exactly the same fp32 distance is dropped (csrc/mr_photon.hip), which the fixtures mark per query (at most 1 %).
The empty map is not queried here: the reference's locate_photons would read a photon nobody stored."""
import importlib.util
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("make_photon_ref", os.path.join(ROOT, "tests", "golden", "make_photon_ref.py"))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)

F = np.float32
U = np.uint32
SINGLE_BATCH = [name for name in gen.PINNED if name not in ("two_batches", "three_batches")]
_cases = {}


def case(name):
    """inputs, fixture and query groups of a case, built once; the inputs are the ones the fixture was recorded on"""
    if name not in _cases:
        import hashlib
        capacity, batches = gen.inputs(name)
        fx = gen.load_fixture(name)
        pw, pos, d = gen.stored_inputs(capacity, batches)
        assert fx["stored"] == len(pos)
        tree_pos = pos[fx["origin"]]
        groups = gen.query_groups(name, tree_pos, fx["plane"])
        assert hashlib.sha256(gen.job_bytes(capacity, batches, groups)).digest() == fx["sha256"], "the seeded inputs changed"
        assert [(g[0], g[1]) for g in groups] == [(g["k"], g["max_dist"]) for g in fx["groups"]]
        _cases[name] = dict(capacity=capacity, batches=batches, fx=fx, pos=tree_pos, groups=groups)
    return _cases[name]


def tied_median(pos, plane):
    """some node with a child has another photon in its subtree with the same pos[plane]; heap order, slot i at row i - 1"""
    n = len(pos)
    for i in range(1, n // 2 + 1):
        axis, sub, level = plane[i - 1], [], np.array([2 * i, 2 * i + 1])
        level = level[level <= n]
        while len(level):
            sub.append(level)
            level = np.concatenate([2 * level, 2 * level + 1])
            level = level[level <= n]
        if (pos[np.concatenate(sub) - 1, axis] == pos[i - 1, axis]).any():
            return True
    return False


def fill(m, batches):
    for pw, pos, d, scale in batches:
        m.store(pw, pos, d)
        m.scale_photon_power(float(scale))
    return m


def oracle_map(oracle, c):
    m = fill(oracle.PhotonMap(c["capacity"]), c["batches"])
    m.balance()
    return m


def product_host_map(miro, c, host_only=True):
    m = fill(miro.PhotonMap(c["capacity"]), c["batches"])
    m.balance(host_only=host_only)
    return m


def assert_tree_is_the_references(exported, c):
    pos, plane, tp, power = exported
    fx, n = c["fx"], c["fx"]["stored"]
    assert len(pos) == n
    assert np.array_equal(pos.view(U), c["pos"].view(U)), "pos"
    assert np.array_equal(power.view(U), fx["power"].view(U)), "power"
    assert np.array_equal(tp, fx["theta_phi"]), "theta_phi"
    inner = 2 * (np.arange(n) + 1) <= n
    assert (fx["plane"][~inner] == -1).all() and np.array_equal(np.asarray(plane)[inner], fx["plane"][inner]), "plane"


def records(pos, tp, power):
    """the photon records of a tree as sortable rows"""
    rows = np.concatenate([pos.view(U), power.view(U), tp.astype(U)], axis=1)
    return rows[np.lexsort(rows.T[::-1])]


# ---- without a GPU -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", gen.CASES)
def test_fixtures_are_what_the_reference_binary_writes(name):
    """Where build() made oracle/_ref/photon_ref (a checkout of the reference was at hand), every stored array is byte for byte
    what the driver computes today from the seeded inputs."""
    if not os.path.exists(gen.BINARY):
        pytest.skip("oracle/_ref/photon_ref is not built here (no checkout of the reference)")
    arrays, _, _ = gen.generate(name, gen.BINARY)
    with np.load(os.path.join(gen.OUT, name + ".npz")) as z:
        assert sorted(z.files) == sorted(arrays)
        for key in z.files:
            want, got = z[key], np.asarray(arrays[key])
            assert want.dtype == got.dtype and want.shape == got.shape and want.tobytes() == got.tobytes(), key


def test_fixture_directory_is_small():
    files = [os.path.join(gen.OUT, f) for f in os.listdir(gen.OUT)]
    assert sorted(os.path.basename(f) for f in files) == sorted(name + ".npz" for name in gen.CASES)
    assert sum(os.path.getsize(f) for f in files) < 1000000


@pytest.mark.parametrize("name", gen.PINNED + gen.EXACT_TIES)
def test_oracle_is_the_reference_without_a_tied_median(oracle, name):
    """tree (pos and power on their uint32 views, direction bytes, planes where 2*i <= n), found, dist2[0] on its uint32 view and
    the irradiance BITWISE -- the oracle sums in the reference's order -- on every query of every group.  On the `mirror` map
    most answers depend on which of two photons at exactly the same distance the reference drops: its heap stops at an equal
    child while it is built and passes one while it inserts, and the oracle has to do both."""
    c = case(name)
    m = oracle_map(oracle, c)
    assert m.count() == c["fx"]["stored"]
    assert_tree_is_the_references(m.export(), c)
    for (k, md, q, qn), g in zip(c["groups"], c["fx"]["groups"]):
        irr, found, r2 = m.irradiance_estimate(q, qn, max_dist=float(md), nphotons=k)
        assert np.array_equal(found, g["found"]), (k, md)
        assert np.array_equal(r2.view(U), g["r2"].view(U)), (k, md)
        assert np.array_equal(irr.view(U), g["irradiance"].view(U)), (k, md)


@pytest.mark.parametrize("name", gen.PINNED + gen.EXACT_TIES)
def test_host_balance_is_the_reference_without_a_tied_median(miro, name):
    """store, scale_photon_power, balance(host_only=True), export: no device needed"""
    c = case(name)
    m = product_host_map(miro, c)
    assert m.count() == c["fx"]["stored"]
    assert_tree_is_the_references(m.export(), c)


@pytest.mark.parametrize("name", gen.CASES)
def test_tied_median_predicate(oracle, name):
    """the same answer on the reference's tree and on the oracle's; false on every pinned map, true on the three deviation maps"""
    c = case(name)
    on_reference = tied_median(c["pos"], c["fx"]["plane"])
    pos, plane, _, _ = oracle_map(oracle, c).export()
    assert on_reference == tied_median(pos, plane) == c["fx"]["tied_median"]
    if name in gen.PINNED + gen.EXACT_TIES:
        assert not on_reference
    if name in gen.TIED:
        assert on_reference


@pytest.mark.parametrize("name", gen.TIED)
@pytest.mark.xfail(strict=True, reason="tied median: the oracle and both product builders select by (coordinate, index), the "
                                       "reference's median_split (a Sedgewick partition) does not; deviation measured in DESIGN.md")
def test_tied_median_tree_is_the_references(oracle, name):
    c = case(name)
    assert_tree_is_the_references(oracle_map(oracle, c).export(), c)


@pytest.mark.parametrize("name", gen.TIED + gen.WALK)
def test_tied_median_maps_hold_the_references_records(oracle, miro, name):
    """What holds with a tied median too: the product's host tree is the oracle's, and both hold the reference's photon records
    -- positions, direction bytes and scaled powers -- as a multiset."""
    c = case(name)
    fx = c["fx"]
    opos, oplane, otp, opw = oracle_map(oracle, c).export()
    ppos, pplane, ptp, ppw = product_host_map(miro, c).export()
    n = fx["stored"]
    assert np.array_equal(ppos.view(U), opos.view(U)) and np.array_equal(ppw.view(U), opw.view(U)) and np.array_equal(ptp, otp)
    inner = np.arange(n) + 1 < n // 2 - 1
    assert np.array_equal(np.asarray(pplane)[inner], np.asarray(oplane)[inner])
    pw, _, _ = gen.stored_inputs(c["capacity"], c["batches"])
    ref_power = fx["power"] if fx["power"] is not None else (pw * c["batches"][0][3]).astype(F)[fx["origin"]]
    want = records(c["pos"], fx["theta_phi"], ref_power)
    assert np.array_equal(records(opos, otp, opw), want)
    assert np.array_equal(records(ppos, ptp, ppw), want)


# ---- on the MI355X -------------------------------------------------------------------------------------------------------
def estimate(m, q, qn, k, md):
    import torch
    dq, dn = torch.from_numpy(q).cuda(), torch.from_numpy(qn).cuda()
    irr = torch.empty((len(q), 3), dtype=torch.float32, device="cuda")
    found = torch.empty(len(q), dtype=torch.int32, device="cuda")
    r2 = torch.empty(len(q), dtype=torch.float32, device="cuda")
    m.irradiance_estimate(dq, dn, len(q), irr, max_dist=float(md), nphotons=k, d_found=found, d_r2=r2)
    torch.cuda.synchronize()
    return irr.cpu().numpy(), found.cpu().numpy(), r2.cpu().numpy()


def expected_irradiance(fx, g):
    """k <= 50: the float64 sum of the scaled powers over the reference's candidate set, over pi * dist2[0]; k = 500: the fixture's"""
    if g["candidates"] is None:
        return g["irradiance"].astype(np.float64)
    live = np.arange(g["candidates"].shape[1])[None, :] < g["found"][:, None]
    pw = fx["power"].astype(np.float64)[np.maximum(g["candidates"], 1) - 1] * live[:, :, None]
    with np.errstate(divide="ignore", invalid="ignore"):
        return pw.sum(axis=1) / (np.pi * g["r2"].astype(np.float64))[:, None]


@pytest.mark.gpu
@pytest.mark.parametrize("name", gen.PINNED)
def test_device_maps_and_estimates_are_the_references(miro, name):
    """The map built by the host calls and by build_device (one batch: that is what it takes): export() is the fixture tree.
    mr_irradiance_estimate on both, every query group: found and dist2[0] equal on EVERY query; the irradiance within 1e-5 of the
    largest expected value (tests/test_photon.py's figure: summation order only) with the same finiteness pattern, on the queries
    the fixture does not mark as exact-distance ties."""
    import torch
    from test_photon_build import records_of
    c = case(name)
    fx = c["fx"]
    maps = [product_host_map(miro, c, host_only=False)]
    if name in SINGLE_BATCH:
        (pw, pos, d, scale), = c["batches"]
        m = miro.PhotonMap(c["capacity"])
        res = m.build_device(torch.from_numpy(records_of(pw, pos, d)).cuda(), len(pos), float(scale))
        torch.cuda.synchronize()
        assert (res["stored"], res["dropped"]) == (fx["stored"], len(pos) - fx["stored"]) and res["deferred"] <= fx["stored"]
        maps.append(m)
    for m in maps:
        assert m.count() == fx["stored"]
        assert_tree_is_the_references(m.export(), c)
    for (k, md, q, qn), g in zip(c["groups"], fx["groups"]):
        want = expected_irradiance(fx, g)
        clean = ~g["tied"]
        assert clean.mean() >= 0.99
        fin = np.isfinite(want)
        scale = max(float(np.abs(want[fin]).max()) if fin.any() else 0.0, 1e-30)
        for m in maps:
            got, found, r2 = estimate(m, q, qn, k, md)
            assert np.array_equal(found, g["found"]), (k, md)
            assert np.array_equal(r2.view(U), g["r2"].view(U)), (k, md)
            assert np.array_equal(np.isfinite(got)[clean], fin[clean]), (k, md)
            with np.errstate(invalid="ignore"):
                err = np.abs(got.astype(np.float64) - want)[clean & fin.all(axis=1)]
            print("%s k=%d max_dist=%g: largest error %.3g of scale %.3g" % (name, k, md, err.max() if err.size else 0.0, scale))
            assert (err <= 1e-5 * scale).all(), (k, md)
