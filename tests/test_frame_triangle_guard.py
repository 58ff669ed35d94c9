"""The rejection guard of the fused frame's uniform leaf loops (mr_traverse.h: tri_surely_rejects / tri_test_guarded, DESIGN.md
section 4 item 24): a wave whose lanes are all SURE, from a division-free sign test on the numerator of beta or of gamma, that
the reference rejects the leaf's triangle goes to the next record without the three divisions.

CPU: the guard modelled in numpy float32 (tools/tri_guard_replay.py: guard_sure) never calls sure what the reference's own
arithmetic -- numpy's IEEE float32 division, the reject test of Triangle.cpp:158 -- accepts.

GPU: a skipped test writes nothing, so primary records, shadow records and pixels of the fused frame stay the batched pipeline's
and the oracle's, byte for byte.  That a case holds both kinds of test -- skipped ones and ones that run the divisions -- is
asserted with the replay of test_frame_uniform_walk.py under the counters of tools/tri_guard_replay.py (GuardCounts), whose hit
per ray must be the kernel's record."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from helpers import product_scene  # noqa: E402
from miro_amd import frame as mframe  # noqa: E402
from miro_amd import scenes  # noqa: E402
from test_frame_uniform_walk import _bits, _desc, _render, _replay, _shadow_waves, cards_desc, triangle_records  # noqa: E402
from tri_guard_replay import K_EPS, GuardCounts, guard_sure, reference_rejects  # noqa: E402

F = np.float32


# ---------------------------------------------------------------------------------------------------------------- CPU
def _never_sure_of_an_accepted_test(pn, nb, ng, ddotn, tmax=np.inf):
    pn, nb, ng, ddotn = (np.asarray(x, F) for x in np.broadcast_arrays(pn, nb, ng, ddotn))
    sure = guard_sure(nb, ng, ddotn)
    reject = reference_rejects(pn, nb, ng, ddotn, F(0), F(tmax))
    bad = np.nonzero(sure & ~reject)[0]
    assert bad.size == 0, (nb[bad[:4]], ng[bad[:4]], ddotn[bad[:4]])
    return sure


def _random_floats(rng, n):
    """every exponent and sign, denormals and zeros included (no inf / NaN)"""
    bits = rng.randint(0, 1 << 32, size=n, dtype=np.uint64).astype(np.uint32)
    x = bits.view(F).copy()
    x[~np.isfinite(x)] = 0
    return x


def test_sure_implies_the_references_reject_on_random_triples():
    rng = np.random.RandomState(168)
    n = 3000000
    sure = _never_sure_of_an_accepted_test(_random_floats(rng, n), _random_floats(rng, n), _random_floats(rng, n), _random_floats(rng, n))
    assert 0.2 < sure.mean() < 0.8                       # the guard decides a good part of them, and not all
    # numerators and denominators of like size: quotients of order one, where a triangle is hit
    d = _random_floats(rng, n)
    with np.errstate(all="ignore"):
        nb = (d * rng.uniform(-1.5, 1.5, n)).astype(F)
        ng = (d * rng.uniform(-1.5, 1.5, n)).astype(F)
    sure = _never_sure_of_an_accepted_test(_random_floats(rng, n), nb, ng, d)
    assert sure.any() and not sure.all()


def _neighbours(x, steps=(-2, -1, 0, 1, 2)):
    b = np.asarray(x, F).view(np.int32)
    return np.stack([(b + s).view(F) for s in steps]).reshape(-1)


def test_quotients_at_the_guards_bound_and_at_the_references():
    rng = np.random.RandomState(7)
    d = np.concatenate([rng.uniform(0.001, 1000.0, 20000), -rng.uniform(0.001, 1000.0, 20000)]).astype(F)
    for q in (-(2.0 ** -13), -1e-4):
        with np.errstate(all="ignore"):
            nb0 = (d * F(q)).astype(F)
        for s in (-3, -2, -1, 0, 1, 2, 3):               # numerators whose quotient is at the bound and a few ulps either side
            nb = (nb0.view(np.int32) + s).view(F)
            with np.errstate(all="ignore"):
                beta = nb / d
            sure = _never_sure_of_an_accepted_test(F(1), nb, F(0), d) | _never_sure_of_an_accepted_test(F(1), F(0), nb, d)
            # the guard is sure exactly where the REAL quotient is below -2^-13: then the rounded one is at most -2^-13
            assert (beta[sure] <= F(-(2.0 ** -13))).all()
            assert not sure[beta > F(-(2.0 ** -13))].any()
            if q == -1e-4:
                assert not sure.any()                    # between -2^-13 and -kEps the guard leaves the decision to the divisions
    # the quotient exactly -2^-13 is not "below": nb * 2^13 == -|d|
    d = F(3.0)
    assert not guard_sure(F(-3.0 * 2.0 ** -13), F(0), d) and guard_sure(np.nextafter(F(-3.0 * 2.0 ** -13), F(-1)), F(0), d)
    assert F(-(2.0 ** -13)) < -K_EPS


def test_special_denominators_and_numerators():
    den = np.array([0.0, -0.0, 1e-45, -1e-45, 1e-39, -1e-39, np.inf, -np.inf, np.nan, 1.0, -1.0, 3e38, -3e38], F)
    num = np.concatenate([_neighbours(F(0), (0,)), np.array([-0.0, 1e-45, -1e-45, 1e-40, -1e-40, 2.0 ** 115, -(2.0 ** 115), 2.0 ** 116, -(2.0 ** 116),
                                                              3e38, -3e38, np.inf, -np.inf, np.nan, 1.0, -1.0], F)])
    D, NB, NG = (x.reshape(-1) for x in np.meshgrid(den, num, num, indexing="ij"))
    sure = _never_sure_of_an_accepted_test(F(1), NB, NG, D)
    for pn in (F(0), F(-1), F(np.inf), F(np.nan)):
        _never_sure_of_an_accepted_test(pn, NB, NG, D)
    # the cases the code comment argues one by one
    g = lambda nb, d: bool(guard_sure(F(nb), F(0), F(d)))
    assert g(-1.0, 0.0) and not g(1.0, 0.0) and g(1.0, -0.0) and not g(-1.0, -0.0)        # nb / +-0 = -inf: sure; +inf: not
    assert not g(0.0, 0.0) and not g(-0.0, 0.0) and not g(0.0, -0.0)                       # 0 / 0 is NaN in the reference
    assert not g(np.nan, 1.0) and not g(-1.0, np.nan)                                      # a NaN fails every compare
    assert not g(-1.0, np.inf) and not g(1.0, -np.inf) and not g(-np.inf, np.inf)          # x / inf = -0 or NaN: never below -eps
    assert g(-(2.0 ** 116), 1.0) and g(2.0 ** 116, -3e38)                                  # nb * k overflows to -inf: still below
    assert g(-1e-45, 1e-45) and not g(-1e-45, 1.0)                                         # a denormal scaled up is exact
    assert sure.any() and not sure.all()


def test_degenerate_triangle_records():
    # a zero normal: ddotn = +-0 for every direction, and the numerators are whatever the edges leave
    rng = np.random.RandomState(3)
    n = 200000
    z = np.where(rng.rand(n) < 0.5, F(0.0), F(-0.0))
    for nb, ng in ((_random_floats(rng, n), _random_floats(rng, n)), (z, z), (_random_floats(rng, n), z)):
        sure = _never_sure_of_an_accepted_test(z, nb, ng, z)
        with np.errstate(all="ignore"):
            assert (sure == (((nb / z) == -np.inf) | ((ng / z) == -np.inf))).all()


# ---------------------------------------------------------------------------------------------------------------- GPU
gpu = pytest.mark.gpu


def _guard_counts(miro, sc, fu, rays, n_waves, shadow=False, hits=None):
    """the replay's counters for the first n_waves waves; the replay's hits are checked against the kernel's by _replay"""
    with GuardCounts(shadow) as g:
        _replay(miro, sc, fu, rays, n_waves=n_waves, hits=hits)
    return g.c


def _both_kinds(c):
    assert c["skipped"] > 0 and c["guarded"] - c["skipped"] > 0, str(c)


SPONZA_VIEWS = {
    # the default view's top rows: arches and columns against the far walls -- waves that straddle an edge, not all sure
    "silhouette": dict(),
    # close to the side wall, at a grazing angle: the hit triangle's neighbours in the leaf are surely rejected
    "wall": dict(eye=(8.0, 1.5, 1.0), lookat=(0.0, 1.0, -4.5), fov=12.0),
}


@gpu
@pytest.mark.parametrize("view", sorted(SPONZA_VIEWS))
def test_sponza_one_pixel_per_wave(miro, oracle, view):
    sc, fu, ref, rays, src = _render(miro, oracle, _desc("sponza", **SPONZA_VIEWS[view]), 32, 18, 64)
    c = _guard_counts(miro, sc, fu, rays, 64)
    _both_kinds(c)
    if view == "silhouette":
        assert c["all_reject"] > c["all_sure"], str(c)           # tests every lane rejects without every lane being sure
    cs = _guard_counts(miro, sc, fu, _shadow_waves(ref, src, fu.n), 64, shadow=True, hits=fu.d_shadow_hits)
    assert cs["tests_in_walks"] > 0, str(cs)          # (the shadow trace guards leaf_step's scalar arm, not its walk's loop)
    _both_kinds(cs)


@gpu
def test_leaf_shapes(miro, oracle):
    d = cards_desc()
    sc, fu, _, rays, _ = _render(miro, oracle, d, 48, 6, 64)
    _, meta, _ = sc.export_tree()
    assert {0, 1, 2, 3, 4, 16} <= set(meta[meta[:, 0] != 0][:, 2].tolist())
    _both_kinds(_guard_counts(miro, sc, fu, rays, 96))


def _degenerate_desc():
    # two cards; next to the first, inside its outline as the camera sees it, a triangle of zero area (B == A: a zero normal) and
    # an edge-on one (in the plane y = 0, which holds the eye: ddotn is a rounding residue of either sign)
    from test_frame_uniform_walk import _card
    objs = _card(0.0, 2)
    a = (-0.2, -0.1, 0.05)
    objs.append(("triangle", a + a + (0.2, 0.3, 0.05), (0, 0, 1) * 3))
    objs.append(("triangle", (-0.3, 0.0, 0.1, 0.3, 0.0, 0.1, 0.0, 0.0, 0.4), (0, 1, 0) * 3))
    objs += _card(1.5, 4)
    return _desc(dict(models=[], floor=None, objects=objs, eye=(0.75, 0.0, 9.0), lookat=(0.75, 0.0, 0.0), up=scenes.UP, fov=15.0,
                      light=(40.0, 0.0, 0.0), wattage=4000.0))


@gpu
def test_edge_on_and_zero_area_triangles_in_the_hit_leaf(miro, oracle):
    d = _degenerate_desc()
    sc, fu, _, rays, _ = _render(miro, oracle, d, 16, 8, 64)
    _, meta, prims = sc.export_tree()
    A, E1, E2, N = triangle_records(sc)
    zero = np.nonzero((N == 0).all(axis=1))[0]
    edge_on = np.nonzero((N[:, 0] == 0) & (N[:, 2] == 0) & (N[:, 1] != 0) & (A[:, 1] == 0))[0]
    assert len(zero) == 1 and len(edge_on) == 1
    with GuardCounts() as g:
        _, pos, _ = _replay(miro, sc, fu, rays, with_walk_hits=True)
    _both_kinds(g.c)
    leaves = meta[meta[:, 0] != 0]
    for k in (int(zero[0]), int(edge_on[0])):            # its leaf holds a triangle that rays hit
        first, cnt = next((int(f), int(n)) for f, n in leaves[:, 1:] if f <= k < f + n)
        assert ((pos >= first) & (pos < first + cnt) & (pos != k)).any(), (k, first, cnt)
    assert not (pos == int(zero[0])).any()


@gpu
@pytest.mark.parametrize("spp", [4, 1])
def test_tiled_frames(miro, oracle, spp):
    sc, fu, _, rays, _ = _render(miro, oracle, _desc("sponza"), 64, 36, spp, tiled=True)
    _both_kinds(_guard_counts(miro, sc, fu, rays, 36 if spp == 1 else 64))


@gpu
@pytest.mark.parametrize("mode", ["any_shadow", "no_shadows"])
def test_shadow_forms(miro, oracle, mode):
    sc, fu, _, rays, _ = _render(miro, oracle, _desc("sponza"), 16, 8, 64, any_shadow=mode == "any_shadow", no_shadows=mode == "no_shadows")
    _both_kinds(_guard_counts(miro, sc, fu, rays, 64))


@gpu
def test_per_object_materials(miro):
    # the per-object-material kernels take no run and carry no guard: their records stay the batched traces'
    d = _desc("cornell")
    sc = miro.Scene(0)
    n = scenes.populate(sc, d)
    mats = [((0.8, 0.2, 0.2), (0, 0, 0), (0, 0, 0), 1.0, 1.0), ((0.2, 0.8, 0.3), (0, 0, 0), (0, 0, 0), 1.0, 1.0)]
    sc.set_materials(mats, (np.arange(n) % 2).astype(np.uint32))
    sc.build(4)
    ref = mframe.FrameRenderer(sc, d, 16, 8, spp=64, tiled=False)
    ref.generate()
    ref.trace_primary()
    ref.make_shadow_rays()
    ref.trace_shadow()
    fu = mframe.FusedFrame(sc, d, 16, 8, spp=64, tiled=False, keep_hits=True)
    fu.step()
    torch.cuda.synchronize()
    n_s = int(ref.d_count.item())
    assert fu.ray_counts() == (ref.n, n_s) and n_s > 0
    assert np.array_equal(_bits(fu.d_hits), _bits(ref.d_hits))
    src = ref.d_src[:n_s].to(torch.int64)
    assert np.array_equal(_bits(fu.d_shadow_hits[src]), _bits(ref.d_shadow_hits[:n_s]))


@gpu
def test_256_lane_frame(miro, oracle):
    # 625 x 256 x 64, the smallest frame that takes the 256-lane build (test_frame_large.py); the first 48 waves are replayed
    sc, fu, _, rays, _ = _render(miro, oracle, _desc("sponza"), 625, 256, 64, sc=product_scene(miro, "sponza"), with_oracle=False)
    assert fu.n > 10000000
    _both_kinds(_guard_counts(miro, sc, fu, rays, 48))
