"""irradiance_kernel (csrc/mr_photon.hip) and the block boxes it reads, in the regimes tests/test_photon.py, test_photon_build.py
and test_gather_level.py do not enter:

  A  maps of 2^18 photons and more: the fourth layer of blocks (layer_base[3], the `child << 6 <= n` cut-off, the 128-entry stack)
  B  launches of more than 102 400 queries: batches of 64 (the 64-lane pre-pass, a guess chain of 64), the seam between the
     64-wide and the 16-wide batches, the ragged last batch, waves that loop over batches, the hand-out counter's re-arm
  C  irradiance_kernel<true>, the counting build behind count_stats(): the plain kernel's results, and counters that add up
  D  device-built maps searched like host-built ones WITH EQUAL WORK COUNTERS, which is what observes their boxes
  E  launches of fewer queries than a workgroup has waves, no query at all, and the map of no photons

The yardstick of A, B and E is the oracle's PhotonMap.irradiance_estimate (a restatement, itself pinned to the reference's own
PhotonMap.cpp on maps without a tied median: tests/test_photon_reference.py), of D the library's own host path, of C the plain kernel on the same map, which A and B tie to the oracle.  `found` must be
np.array_equal and the radius equal on its uint32 view in every comparison; the irradiance within 1e-5 of the largest expected
value (test_irradiance_estimate_matches_oracle's figure for summation order) with the same finiteness pattern.

Positions are tie-free (random, every coordinate distinct on its axis) wherever powers are non-uniform, powers uniform wherever
positions are tied: which of two photons at exactly the same distance is dropped is not reproduced (csrc/mr_photon.hip's header).
Not pinned here either: the -0 / +0 identity of box corners, the reference's tree on maps with a tied median.  No test
asserts a speed."""
import numpy as np
import pytest

from test_photon import photon_fuzz_case
from test_photon_build import device_map, host_map, same_export, tied_inputs, unit_rows

F = np.float32
U = np.uint32
L4 = 1 << 18                    # the first map size with a fourth layer of blocks (launch_irradiance)
TAIL = 102400                   # kTailQueries: the queries ahead of the last TAIL go out in batches of 64, the rest in 16s
COUNTERS = 16                   # kPhotonWorkCounters: a map's launches take its hand-out counters in turn
SPAN = 8.0
A_PARAMS = [(1, 1e10), (5, 1e10), (50, 1e10), (500, 1e10), (500, 0.15)]


# ---- construction ----------------------------------------------------------------------------------------------------------
def tie_free_positions(rng, n, span):
    """uniform in [0, span)^3 with no two photons sharing a coordinate on any axis (no tied median at balance time)"""
    pos = (rng.rand(n, 3) * span).astype(F)
    for c in range(3):
        while True:
            _, first = np.unique(pos[:, c], return_index=True)
            dup = np.setdiff1d(np.arange(n), first)
            if dup.size == 0:
                break
            pos[dup, c] = (rng.rand(dup.size) * span).astype(F)
    return pos


def random_photons(n, seed, span=SPAN):
    """(power, pos, direction): tie-free positions, random unit directions, non-uniform powers"""
    rng = np.random.RandomState(seed)
    pos = tie_free_positions(rng, n, span)
    return rng.rand(n, 3).astype(F), pos, unit_rows(rng, n)


def oracle_map(oracle, pw, pos, d, scale):
    m = oracle.PhotonMap(len(pos) + 10)
    m.store(pw, pos, d)
    m.scale_photon_power(scale)
    m.balance()
    return m


def dequantised(tp):
    """the direction a photon's two bytes stand for (PhotonMap.cpp:66-71)"""
    th, ph = tp[:, 0].astype(np.float64) / 256.0 * np.pi, tp[:, 1].astype(np.float64) / 256.0 * 2 * np.pi
    return np.stack([np.sin(th) * np.cos(ph), np.sin(th) * np.sin(ph), np.cos(th)], axis=1).astype(F)


def unit(v):
    return (v / np.maximum(np.linalg.norm(v, axis=1, keepdims=True), 1e-20)).astype(F)


def mixture_queries(rng, pos, d, span, nq=640):
    """test_photon_search_fuzz's mixture: on photons, near them, far outside the map, and a random-walk run"""
    n = len(pos)
    q = pos[rng.randint(0, n, nq)].copy()
    kind = rng.randint(0, 4, nq)
    q[kind == 1] += rng.normal(0, span * 0.01, (int((kind == 1).sum()), 3)).astype(F)
    q[kind == 2] = (rng.rand(int((kind == 2).sum()), 3) * span * 3 - span).astype(F)
    run = np.cumsum(rng.normal(0, span * 1e-3, (nq, 3)), axis=0).astype(F)
    q[kind == 3] = (pos[0] + run)[kind == 3]
    qn = -d[rng.randint(0, n, nq)]
    flip = rng.rand(nq) < 0.2
    qn[flip] = rng.normal(size=(int(flip.sum()), 3)).astype(F)
    return np.ascontiguousarray(q, F), unit(qn)


def walk_queries(rng, nq, span, step, jumps=0.0, nan=0.0, origin=None):
    """a random walk of `step` * span per query, folded back into [0, span]^3; a share `jumps` of the queries start again at a
    uniform random point; a share `nan` of the normals is NaN, the frame driver's "no query here" """
    inc = np.cumsum(rng.normal(0, step * span, (nq, 3)), axis=0)
    jump = rng.rand(nq) < jumps
    jump[0] = True
    start = rng.rand(nq, 3) * span
    if origin is not None:
        start[0] = origin
    at = np.maximum.accumulate(np.where(jump, np.arange(nq), 0))     # where this query's run began
    p = start[at] + inc - inc[at]
    p = span - np.abs(np.mod(p, 2 * span) - span)                    # reflect at the walls: neighbours stay neighbours
    qn = unit(np.cumsum(rng.normal(0, 0.05, (nq, 3)), axis=0) + rng.normal(size=3))
    if nan:
        qn[rng.rand(nq) < nan] = np.nan
    return np.ascontiguousarray(p, F), qn


def to_device(q, qn):
    import torch
    return torch.from_numpy(np.ascontiguousarray(q, F)).cuda(), torch.from_numpy(np.ascontiguousarray(qn, F)).cuda()


def product_estimate(m, dq, dn, k, md, nq=None):
    """(irradiance, found, radius) of one estimate launch on device tensors"""
    import torch
    nq = len(dq) if nq is None else nq
    irr = torch.empty((nq, 3), dtype=torch.float32, device="cuda")
    found = torch.empty(nq, dtype=torch.int32, device="cuda")
    r2 = torch.empty(nq, dtype=torch.float32, device="cuda")
    m.irradiance_estimate(dq, dn, nq, irr, max_dist=md, nphotons=k, d_found=found, d_r2=r2)
    torch.cuda.synchronize()
    return irr.cpu().numpy(), found.cpu().numpy(), r2.cpu().numpy()


def assert_same(got, want, what, bytes_equal=False):
    """found and the radius equal on every query, finiteness equal, irradiance within 1e-5 of the largest expected value"""
    (gi, gf, gr), (wi, wf, wr) = got, want
    bad = np.nonzero((gf != wf) | (gr.view(U) != wr.view(U)))[0]
    assert bad.size == 0, "%s: %d queries differ, first %s: found %s vs %s, r2 %s vs %s" % (
        what, bad.size, bad[:5], gf[bad[:5]], wf[bad[:5]], gr[bad[:5]], wr[bad[:5]])
    fin = np.isfinite(wi)
    assert np.array_equal(np.isfinite(gi), fin), what
    if bytes_equal:
        assert np.array_equal(gi.view(U), wi.view(U)), what
    elif fin.any():
        scale = float(np.abs(wi[fin]).max())
        err = float(np.abs(gi[fin].astype(np.float64) - wi[fin].astype(np.float64)).max())
        assert err <= 1e-5 * scale, "%s: irradiance off by %g of the largest expected value" % (what, err / max(scale, 1e-300))


@pytest.fixture(scope="module")
def big_maps(oracle, miro):
    """maps of about 2^18 photons, built once per size: (oracle map, resident product map, heap-ordered pos, direction bytes)"""
    cache = {}

    def get(n):
        if n not in cache:
            pw, pos, d = random_photons(n, 1000 + n % 997)
            a = oracle_map(oracle, pw, pos, d, 1.0 / n)
            b = host_map(miro, pw, pos, d, 1.0 / n, host_only=False)
            hpos, _, tp, _ = a.export()
            cache[n] = (a, b, hpos, tp)
        return cache[n]
    return get


# ---- A: four layers --------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("n", [L4 - 1, L4, L4 + 1, L4 + 3, L4 + 63, L4 + 64, L4 + 4159, 330000])
def test_four_layers_match_the_oracle(oracle, miro, big_maps, n):
    """2^18 - 1 is the last three-layer map; 2^18 ... 2^18 + 3 hold a fourth-layer block whose photons locate_photons never
    reaches (their parent's index is >= n/2 - 1); the rest have a populated, ragged fourth layer.  Query sets: (a) ON photons of
    heap slots >= 2^18 and on the heap's last 8, each facing its photon; (b) the fuzz's mixture; (c) a random walk of 1e-3 of the
    span per query (the guessed radius).  With k = 500 inside 0.15 every set-(a) query on a reachable photon of a map of
    2^18 + 63 or more finds something: fourth-layer photons are in the result."""
    a, b, hpos, tp = big_maps(n)
    rng = np.random.RandomState(n % 1009)
    last = np.arange(n - 7, n + 1)                                   # heap slots, 1-based
    deep = np.arange(L4, n + 1)
    if deep.size > 632:
        deep = rng.choice(deep, 632, replace=False)
    slots = np.unique(np.concatenate([deep, last]))
    assert slots.size <= 640
    unreachable_last = (last >> 1) >= n // 2 - 1
    assert unreachable_last.any() and not unreachable_last.all()
    ddir = dequantised(tp)
    sets = {"a": (hpos[slots - 1].copy(), -ddir[slots - 1]),
            "b": mixture_queries(rng, hpos, ddir, SPAN),
            "c": walk_queries(rng, 640, SPAN, 1e-3, origin=hpos[rng.randint(0, n)])}
    for name, (q, qn) in sets.items():
        dq, dn = to_device(q, qn)
        for k, md in A_PARAMS:
            want = a.irradiance_estimate(q, qn, max_dist=md, nphotons=k)
            assert_same(product_estimate(b, dq, dn, k, md), want, "n=%d set %s k=%d md=%g" % (n, name, k, md))
            if name == "a" and (k, md) == (500, 0.15) and n >= L4 + 63:
                reachable = (slots >> 1) < n // 2 - 1
                in_fourth = reachable & (slots >= L4)
                assert in_fourth.sum() >= 32 and (want[1][reachable] >= 1).all()
            if name == "c" and md == 1e10:
                assert (want[1] == k).all()                          # every query overflows: a guess follows a guess


FOUR_LAYER_FUZZ_SIZES = (L4 - 2, L4 - 1, L4, L4 + 1, L4 + 2, 300000)


@pytest.mark.gpu
@pytest.mark.parametrize("seed", [24, 25])
def test_photon_search_fuzz_four_layers(oracle, miro, seed):
    """test_photon_search_fuzz's generator (grid positions with uniform powers included) with the map size drawn from around 2^18
    and 300 000, irradiance within 1e-5: the two seeds after test_photon_search_fuzz's own.  Seed 24 draws a generic map of 2^18
    photons, seed 25 a grid map of 2^18 + 1 (asserted in the no-GPU test below)."""
    photon_fuzz_case(oracle, miro, seed, sizes=FOUR_LAYER_FUZZ_SIZES, jitter=False, tol=1e-5)


# ---- B: more than 102 400 queries in one launch ----------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small_maps(oracle, miro):
    cache = {}

    def get(n):
        if n not in cache:
            pw, pos, d = random_photons(n, 77 + n, span=1.0)
            cache[n] = (oracle_map(oracle, pw, pos, d, 1.0 / n), host_map(miro, pw, pos, d, 1.0 / n, host_only=False))
        return cache[n]
    return get


def nan_rule(want, qn):
    """what the kernel defines for a NaN normal: irradiance 0, found 0, radius 0.0.  The oracle finds nothing there either (no
    photon faces a NaN normal); its radius stays max_dist^2 and its irradiance 0."""
    skip = np.isnan(qn[:, 0])
    wi, wf, wr = (x.copy() for x in want)
    assert (wf[skip] == 0).all()
    wi[skip], wr[skip] = 0.0, 0.0
    return (wi, wf, wr), skip


B_CASES = [(n, k, nq) for n, k in ((5000, 1), (5000, 8), (300, 500)) for nq in (TAIL + 1, TAIL + 64, TAIL + 64 * 3 + 21)]
B_CASES.append((5000, 8, TAIL + 64 * 1600))


@pytest.mark.gpu
@pytest.mark.parametrize("n,k,nq", B_CASES)
def test_long_launches_match_the_oracle(oracle, miro, small_maps, n, k, nq):
    """nq = 102 400 + 1: no batch of 64; + 64: exactly one; + 64 * 3 + 21: three and a ragged last small batch; + 64 * 1 600: more
    batches than the 1 536 workgroups' waves, which loop, and the re-arm with a capped grid.  Queries: a random walk of 8e-3 per
    step inside the map, 5 % jumps, 3 % NaN normals.  The 300-photon map with k = 500 never overflows and so never guesses.
    Afterwards 16 launches of 17 queries on the same map (the 16th takes the long launch's hand-out counter again: it answers
    nothing, or not everything, if that counter was not re-armed)."""
    a, b = small_maps(n)
    rng = np.random.RandomState(nq % 100003 + k)
    q, qn = walk_queries(rng, nq, 1.0, 8e-3, jumps=0.05, nan=0.03)
    want, skip = nan_rule(a.irradiance_estimate(q, qn, max_dist=1e10, nphotons=k), qn)
    assert 0.02 < skip.mean() < 0.04
    full = want[1][~skip] == k
    overflow = full & (want[2][~skip] != F(1e10) * F(1e10))
    print("n=%d k=%d nq=%d: %.1f %% of the queries find k, %.1f %% overflow" % (n, k, nq, 100 * full.mean(), 100 * overflow.mean()))
    if n == 5000:
        assert full.mean() >= 0.5
    else:
        assert not overflow.any()
    if k == 1:                                                       # the first-overflow quirk is live
        brute = a.irradiance_estimate(q[:3000], qn[:3000], max_dist=1e10, nphotons=k, brute=True)
        differ = (want[2][:3000].view(U) != brute[2].view(U))[~skip[:3000]]
        print("k=1: the first-overflow replacement changes %.1f %% of the answers" % (100 * differ.mean()))
        assert 0.01 < differ.mean() < 0.9
    dq, dn = to_device(q, qn)
    got = product_estimate(b, dq, dn, k, 1e10)
    assert (got[0][skip] == 0).all() and (got[1][skip] == 0).all() and (got[2][skip] == 0).all()
    assert_same(got, want, "n=%d k=%d nq=%d" % (n, k, nq))
    few = slice(1000, 1017)
    want_few = tuple(x[few] for x in want)
    dq, dn = to_device(q[few], qn[few])
    for i in range(COUNTERS):
        assert_same(product_estimate(b, dq, dn, k, 1e10), want_few, "launch %d of 17 queries after nq=%d" % (i, nq))


# ---- C: the counting kernel ------------------------------------------------------------------------------------------------
def counter_identities(s, found, n_queries, what):
    assert s["queries"] == n_queries, what
    assert s["unguessed"] <= s["queries"], what
    assert s["repeated_searches"] <= s["queries"] - s["unguessed"], what
    assert s["candidates"] >= int(found.sum()), what
    assert s["records_searched"] <= 63 * s["blocks"], what
    assert s["boxes_measured"] <= 64 * s["expansions"], what
    assert s["unused9"] == 0 and s["unused11"] == 0, what


def counted(m, dq, dn, k, md):
    """one launch of the counting kernel on a map with count_stats on: (results, its counters); the counters are zero after"""
    m.stats(reset=True)
    out = product_estimate(m, dq, dn, k, md)
    s = m.stats(reset=True)
    assert not any(m.stats().values())
    return out, s


@pytest.mark.gpu
@pytest.mark.parametrize("n", [50, 20000, L4 + 4159])
def test_counting_kernel(miro, big_maps, n):
    """irradiance_kernel<true> against irradiance_kernel<false> on the same map and queries -- plain, counting, counting again,
    plain again after count_stats(False) --: found, radius AND the irradiance's bytes are equal across all four (the two
    instantiations add the same candidates in the same order), and the second counting launch reproduces every counter: batches are
    a fixed partition of the query indices and a guess chain never leaves its batch.  The counters obey what the code implies; no
    magnitude is asserted (the observed ones are in profiles/photon_regimes.log).  A map of fewer than 64 photons has one block
    and expands nothing."""
    if n >= L4:
        m, span = big_maps(n)[1], SPAN
        hpos, ddir = big_maps(n)[2], dequantised(big_maps(n)[3])
    else:
        pw, pos, d = random_photons(n, 500 + n)
        m, span = host_map(miro, pw, pos, d, 1.0 / n, host_only=False), SPAN
        hpos, _, tp, _ = m.export()
        ddir = dequantised(tp)
    rng = np.random.RandomState(31 + n % 1009)
    sets = {"mixture": mixture_queries(rng, hpos, ddir, span),
            "walk": walk_queries(rng, TAIL + 64 * 3 + 21, span, 8e-3, jumps=0.05, nan=0.03)}
    for name, (q, qn) in sets.items():
        dq, dn = to_device(q, qn)
        live = int((~np.isnan(qn[:, 0])).sum())
        for k in (4, 50, 500):
            for md in (1e10, 0.15):
                what = "n=%d %s k=%d md=%g" % (n, name, k, md)
                plain = product_estimate(m, dq, dn, k, md)
                m.count_stats(True)
                first, s1 = counted(m, dq, dn, k, md)
                second, s2 = counted(m, dq, dn, k, md)
                m.count_stats(False)
                again = product_estimate(m, dq, dn, k, md)
                for other in (first, second, again):
                    assert_same(other, plain, what, bytes_equal=True)
                counter_identities(s1, plain[1], live, what)
                assert s2 == s1, what
                assert n >= 64 or s1["expansions"] == 0
                print(what, s1)
    with pytest.raises(miro.MiroError):
        m.stats()                                                    # counting is off again


# ---- D: device-built maps --------------------------------------------------------------------------------------------------
D_SIZES = [0, 1, 2, 63, 64, 65, 127, 128, 4095, 4096, 4097, 4159, 8191, 70001, L4 - 1, L4, L4 + 65]
D_CASES = D_SIZES + ["plane", "point", "lattice", "four_x", "grid", "far"]


def d_inputs(case):
    """(power, pos, direction, tie_free)"""
    if isinstance(case, int):
        return random_photons(case, 900 + case % 991) + (True,)
    if case == "far":                                                # every position beyond 1e8, as test_capping_and_state has it
        rng = np.random.RandomState(13)
        pos = (rng.rand(200, 3).astype(F) * F(1e9) + F(2e8)).astype(F)
        pos[:, 1] = -pos[:, 1]
        return rng.rand(200, 3).astype(F), pos, unit_rows(rng, 200), False
    if case == "grid":                                               # the fuzz's coarse grid: coincident photons, and queries whose
        rng = np.random.RandomState(17)                              # distance to a box equals their radius to the bit
        pos = (rng.randint(0, 17, (20000, 3)) * 0.5).astype(F)
        return np.full((20000, 3), 0.25, F), pos, unit_rows(rng, 20000), False
    _, pos, d = tied_inputs(case)
    return np.full((len(pos), 3), 0.25, F), pos, d, False            # tied positions: uniform powers


@pytest.mark.gpu
@pytest.mark.parametrize("case", D_CASES, ids=str)
def test_device_built_maps_search_like_host_built_ones(oracle, miro, case):
    """build_device against store / scale / balance on the same records: same_export, and the same <= 640 queries (on photons,
    near them, outside the map) with counting on -- found and radius equal, irradiance within tolerance and ALL TWELVE COUNTERS
    equal.  The counters are what holds the boxes: a box that is looser or tighter than the host's changes `blocks`,
    `boxes_measured` or `records_searched` even where the answers survive.  Sizes around the block boundaries 64, 4096 and 2^18,
    ragged last levels, tied_inputs, a coarse grid, positions beyond 1e8.  How sharp this is: a box changes a counter when some
    query's radius falls between the two boxes' distances, so on generic positions an error of one ulp goes unseen; on the
    lattice and the grid, where a query's distance to a box often EQUALS its radius (the comparison is strict), one ulp shows.
    Not observable this way, and not claimed: whether a box corner is -0 or +0.  On the tie-free sizes the device-built map's
    estimates are also the oracle's."""
    pw, pos, d, tie_free = d_inputs(case)
    n = len(pos)
    scale = 1.0 / n if n else 1.0
    dev, res = device_map(miro, pw, pos, d, scale)
    assert (res["stored"], res["dropped"]) == (n, 0)
    host = host_map(miro, pw, pos, d, scale, host_only=False)
    same_export(dev, host)
    lo = pos.min(axis=0).astype(np.float64) if n else np.zeros(3)
    span = float((pos.max(axis=0).astype(np.float64) - lo).max()) if n else 1.0
    span = span if span > 0 else 1.0
    rng = np.random.RandomState(5 + n % 1013)
    nq = 640
    kind = rng.randint(0, 3, nq) if n else np.full(nq, 2)
    q = pos[rng.randint(0, n, nq)].astype(np.float64) if n else np.zeros((nq, 3))
    q[kind == 1] += rng.normal(0, span * 0.01, (int((kind == 1).sum()), 3))
    q[kind == 2] = lo + rng.rand(int((kind == 2).sum()), 3) * span * 3 - span
    q = q.astype(F)
    qn = -d[rng.randint(0, n, nq)] if n else rng.normal(size=(nq, 3))
    flip = rng.rand(nq) < 0.2
    qn[flip] = rng.normal(size=(int(flip.sum()), 3))
    qn = unit(qn)
    dq, dn = to_device(q, qn)
    ref = oracle_map(oracle, pw, pos, d, scale) if tie_free and n >= 1 else None
    dev.count_stats(True)
    host.count_stats(True)
    for k, md in ((1, 1e10), (9, span / 10), (200, 1e10)):
        what = "%s k=%d md=%g" % (case, k, md)
        want, sh = counted(host, dq, dn, k, md)
        got, sd = counted(dev, dq, dn, k, md)
        assert_same(got, want, what)
        assert sd == sh, "%s: counters (device-built, host-built) %s" % (what, {c: (sd[c], sh[c]) for c in sd if sd[c] != sh[c]})
        assert sh["queries"] == nq
        if ref is not None:
            assert_same(got, ref.irradiance_estimate(q, qn, max_dist=md, nphotons=k), what + " (oracle)")


# ---- E: small launches and the empty map -----------------------------------------------------------------------------------
@pytest.mark.gpu
def test_small_launches(oracle, miro):
    """1 ... 65 queries on a map of 4 097 photons: fewer queries than a workgroup has waves, one batch and a ragged one, one
    workgroup and a few; twice through the list, so that hand-out counters come round again.  No query at all: OK, and nothing
    written."""
    import torch
    n = 4097
    pw, pos, d = random_photons(n, 4097)
    a, b = oracle_map(oracle, pw, pos, d, 1.0 / n), host_map(miro, pw, pos, d, 1.0 / n, host_only=False)
    rng = np.random.RandomState(65)
    q, qn = mixture_queries(rng, pos, d, SPAN, nq=65)
    dq, dn = to_device(q, qn)
    for k, md in ((7, 1e10), (500, 1.5)):
        want = a.irradiance_estimate(q, qn, max_dist=md, nphotons=k)
        for nq in (1, 2, 3, 4, 5, 15, 16, 17, 63, 64, 65) * 2:
            assert_same(product_estimate(b, dq, dn, k, md, nq=nq), tuple(x[:nq] for x in want), "nq=%d k=%d" % (nq, k))
    irr = torch.full((4, 3), -7.0, dtype=torch.float32, device="cuda")
    found = torch.full((4,), -7, dtype=torch.int32, device="cuda")
    r2 = torch.full((4,), -7.0, dtype=torch.float32, device="cuda")
    b.irradiance_estimate(dq, dn, 0, irr, max_dist=1e10, nphotons=7, d_found=found, d_r2=r2)
    torch.cuda.synchronize()
    assert (irr == -7).all() and (found == -7).all() and (r2 == -7).all()
    assert_same(product_estimate(b, dq, dn, 7, 1e10), a.irradiance_estimate(q, qn, max_dist=1e10, nphotons=7), "after nq=0")


@pytest.mark.gpu
@pytest.mark.parametrize("built", ["host", "device"])
def test_empty_map(oracle, miro, built):
    """A balanced map of no photons: found 0, irradiance 0 and the radius max_dist^2 (PhotonMap.cpp:99-136: np.dist2[0] starts as
    max_dist^2 and nothing is ever offered), which is what the oracle gives for an empty map"""
    none = np.zeros((0, 3), F)
    m = host_map(miro, none, none, none, 1.0, host_only=False) if built == "host" else device_map(miro, none, none, none, 1.0)[0]
    assert m.count() == 0
    a = oracle.PhotonMap(10)
    a.balance()
    rng = np.random.RandomState(3)
    q, qn = rng.rand(70, 3).astype(F), unit_rows(rng, 70)
    dq, dn = to_device(q, qn)
    for k, md in ((1, 1e10), (500, 0.15)):
        got = product_estimate(m, dq, dn, k, md)
        assert (got[0] == 0).all() and (got[1] == 0).all() and (got[2].view(U) == (F(md) * F(md)).view(U)).all()
        assert_same(got, a.irradiance_estimate(q, qn, max_dist=md, nphotons=k), "empty map, %s-built, k=%d" % (built, k))


# ---- without a GPU ---------------------------------------------------------------------------------------------------------
def test_inputs_are_what_the_docstrings_say():
    """the constructions above, checked where no device is needed: tie-free positions have distinct coordinates on every axis,
    the walk stays inside the map and keeps neighbours near, the two four-layer fuzz seeds draw a grid and a generic map"""
    pw, pos, d = random_photons(70001, 3)
    assert all(np.unique(pos[:, c]).size == len(pos) for c in range(3))
    assert np.abs(np.linalg.norm(d, axis=1) - 1).max() < 1e-6
    rng = np.random.RandomState(1)
    q, qn = walk_queries(rng, 5000, 8.0, 8e-3, jumps=0.05, nan=0.03)
    assert q.min() >= 0 and q.max() <= 8 and 0.02 < np.isnan(qn[:, 0]).mean() < 0.04
    step = np.linalg.norm(np.diff(q.astype(np.float64), axis=0), axis=1)
    assert 0.03 < (step > 0.5).mean() < 0.07 and np.median(step) < 0.2
    drawn = []
    for seed in (24, 25):
        g = np.random.default_rng(4242 + seed)                       # photon_fuzz_case's first draws
        size = int(g.choice(FOUR_LAYER_FUZZ_SIZES))
        if g.random() < 0.5:
            g.integers(-3, 4)
        g.choice([1, 2, 7, 50, 200, 500, 512])
        drawn.append((size, bool(g.random() < 0.6)))
    assert drawn == [(L4, False), (L4 + 1, True)]
