"""BVH::build on the device (mr_build_opts.builder = MR_BUILD_REFERENCE_DEVICE, csrc/mr_bvh_build.hip): the tree of the host
builder, bit for bit.

The yardstick everywhere is the library's own host builder (builder = 0), which test_host_parity.py pins to the oracle and the
oracle to the reference's counters.  "Same tree" (same_tree below): export_tree()'s corners equal on their uint32 views, meta3 and
leaf_prims array_equal, info()'s n_nodes / n_leaves / max_depth equal.  On every finite scene build_timing() must also name
builder 1: a silent hand-over to the host would make every comparison pass while testing nothing.  No test asserts a time."""
import os
import re
import sys

import numpy as np
import pytest

from helpers import random_rays
from miro_amd import scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import kernel_budget  # noqa: E402

F = np.float32
HOST, DEVICE = 0, 1


# ---- without a GPU ---------------------------------------------------------------------------------------------------------
def test_symbols_and_prototypes(miro):
    from miro_amd import binding
    strip = lambda name: re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", name)).read(), flags=re.S)
    assert re.search(r"MR_BUILD_REFERENCE_DEVICE\s*=\s*1\b", strip("miro_hip.h"))
    assert binding.MR_BUILD_REFERENCE == 0 and binding.MR_BUILD_REFERENCE_DEVICE == 1
    assert re.search(r"\bmr_status\s+mr_bvh_build_timing\s*\(\s*uint32_t\s*\*\s*builder_used\s*,\s*double\s*\*\s*prims_ms\s*,\s*double\s*\*\s*levels_ms"
                     r"\s*,\s*double\s*\*\s*finish_ms\s*,\s*double\s*\*\s*upload_ms\s*\)", strip("miro_hip_surface.h"))
    assert not re.search(r"\bmr_bvh_build_timing\s*\(", strip("miro_hip.h"))
    assert "mr_bvh_build_timing" in binding.SURFACE_SYMBOLS and "mr_bvh_build_timing" not in binding.EXPORTED_SYMBOLS
    assert len(binding.EXPORTED_SYMBOLS) == 69
    assert hasattr(miro.lib(), "mr_bvh_build_timing") and hasattr(miro.Scene, "build_timing")
    # every pointer may be NULL
    assert miro.lib().mr_bvh_build_timing(None, None, None, None, None) == binding.MR_OK


def test_argument_errors_come_before_any_device_call(miro):
    """This runs on a machine without a device: a refusal that needed one would read "no HIP device available"."""
    from miro_amd import binding
    s = miro.Scene()
    s.add_triangle([0, 0, 0, 1, 0, 0, 0, 1, 0], [0, 0, 1] * 3)
    for host_only in (False, True):
        with pytest.raises(miro.MiroError) as e:
            s.build(4, host_only=host_only, builder=2)
        assert e.value.status == binding.MR_ERR_INVALID and "unknown builder 2" in str(e.value)
    with pytest.raises(miro.MiroError) as e:
        s.build(4, host_only=True, builder=DEVICE)
    assert e.value.status == binding.MR_ERR_INVALID and "host_only" in str(e.value)
    # the refused calls left the scene as it was: the host builder still builds it
    assert s.build(4, host_only=True).n_nodes == 1


def test_kernels_stay_inside_the_envelope_verified_on_the_gpu():
    """The six kernels of mr_bvh_build.hip (the level kernel in its four-wave and its one-wave form): inside
    tests/golden/kernel_budget_bvh_build.json (written from the build whose GPU run of this file was green) and the worst values
    of tests/golden/kernel_budget.json; no scratch and no spilled VGPR at all."""
    cur = kernel_budget.unit_kernels("mr_bvh_build")
    assert len(cur) == 6
    for word, forms in (("bvh_objects_kernel", 1), ("bvh_level_kernel", 2), ("bvh_sizes_kernel", 1), ("bvh_preorder_kernel", 1), ("bvh_emit_kernel", 1)):
        assert sum(word in k for k in cur) == forms, word
    kernel_budget.assert_inside_envelope(cur, "kernel_budget_bvh_build.json")
    for name, c in cur.items():
        assert c["scratch_bytes_per_lane"] == 0 and c["vgprs_spilled"] == 0, (name, c)


# ---- on the MI355X ---------------------------------------------------------------------------------------------------------
def same_tree(a, b):
    ca, ma, pa = a.export_tree()
    cb, mb, pb = b.export_tree()
    ia, ib = a.info(), b.info()
    assert (ia.n_nodes, ia.n_leaves, ia.max_depth) == (ib.n_nodes, ib.n_leaves, ib.max_depth)
    assert ca.shape == cb.shape and np.array_equal(ca.view(np.uint32), cb.view(np.uint32))
    assert np.array_equal(ma, mb)
    assert np.array_equal(pa, pb)


def both_builders(miro, fill, leaf, finite=True):
    """(host-built scene, device-built scene) of the same construction steps; checks which builder produced the second"""
    host, dev = miro.Scene(), miro.Scene()
    fill(host)
    fill(dev)
    host.build(leaf, host_only=True)
    assert host.build_timing()["builder"] == HOST
    dev.build(leaf, builder=DEVICE)
    assert dev.build_timing()["builder"] == (DEVICE if finite else HOST)
    return host, dev


def mesh_filler(v, f):
    v = np.asarray(v, F).reshape(-1, 3)
    f = np.asarray(f, np.uint32).reshape(-1, 3)
    n = np.tile(np.asarray([[0, 0, 1]], F), (max(len(v), 1), 1))
    return lambda s: s.add_arrays(v, n[:len(v)], f, f) if len(f) else None


def degenerate_cases():
    """the inputs of test_host_parity.test_builder_degenerate_inputs"""
    cases = {"empty": (np.zeros((0, 3), F), np.zeros((0, 3), np.uint32)),
             "one": ([[0, 0, 0], [1, 0, 0], [0, 1, 0]], [[0, 1, 2]])}
    vs, fs = [], []
    for k in range(40):      # one centroid: every split puts all of them on one side, down to depth 32
        vs += [[0.25, 0.5, -1.0], [1.5, 0.125, 0.75], [-0.5, 2.0, 0.5]]
        fs.append([3 * k, 3 * k + 1, 3 * k + 2])
    cases["coincident"] = (vs, fs)
    g = [[x, 0, z] for x in range(13) for z in range(13)]
    f = []
    for x in range(12):
        for z in range(12):
            a0 = x * 13 + z
            f += [[a0, a0 + 13, a0 + 14], [a0, a0 + 14, a0 + 1]]
    cases["flat_grid"] = (g, f)
    return cases


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["empty", "one", "coincident", "flat_grid"])
def test_degenerate_inputs(miro, name):
    v, f = degenerate_cases()[name]
    host, dev = both_builders(miro, mesh_filler(v, f), 4)
    same_tree(host, dev)
    if name == "coincident":
        assert dev.info().max_depth == 32            # with an empty sibling at every depth
        _, meta, _ = dev.export_tree()
        assert ((meta[:, 0] == 1) & (meta[:, 2] == 0)).sum() == 32
    if name in ("empty", "one"):
        assert dev.info().n_nodes == 1


@pytest.mark.gpu
@pytest.mark.parametrize("leaf", [1, 2, 4, 8])
@pytest.mark.parametrize("n", [4, 5])
def test_leaf_size_edges(miro, n, leaf):
    rng = np.random.default_rng(100 * n + leaf)
    v = (rng.random((3 * n, 3)) * 4 - 2).astype(F)
    f = np.arange(3 * n, dtype=np.uint32).reshape(-1, 3)
    host, dev = both_builders(miro, mesh_filler(v, f), leaf)
    same_tree(host, dev)
    if leaf == 4:
        assert dev.info().n_nodes == (1 if n == 4 else 3)


@pytest.mark.gpu
@pytest.mark.parametrize("name,leaf", [("cornell", 4), ("teapot", 4), ("teapot", 8), ("sphere", 4), ("testobj", 4), ("spiral", 4),
                                       ("bunny", 4), ("bunny", 8), ("sponza", 4)])
def test_named_scenes(miro, name, leaf):
    host, dev = both_builders(miro, lambda s: scenes.populate(s, name), leaf)
    same_tree(host, dev)


def replay(s, steps):
    for st in steps:
        if st[0] == "mesh":
            s.add_arrays(st[1], st[2], st[3], st[3])
        elif st[0] == "sphere":
            s.add_sphere(st[1], st[2])
        else:
            s.add_plane(st[1], st[2])


@pytest.mark.gpu
@pytest.mark.parametrize("seed", range(8))
def test_fuzz_scenes(miro, seed):
    """The generator of test_gpu_fuzz: grid soups, duplicates, zero-area triangles, spheres and all four leaf sizes produce cost
    ties and centroids equal to planes."""
    from test_gpu_fuzz import BASE, make_scene
    steps, leaf, _ = make_scene(np.random.default_rng(BASE + seed))
    host, dev = both_builders(miro, lambda s: replay(s, steps), leaf)
    same_tree(host, dev)


def bisection_planes(lo, hi, steps):
    """every plane the bisection of [lo, hi] can visit in its first `steps` steps, computed as bisect_axis does, in fp32"""
    two = F(2)
    out, frontier = [], [(F(lo), F(hi))]
    for _ in range(steps + 1):
        nxt = []
        for a, b in frontier:
            p = F(F(a + b) / two)
            out.append(p)
            nxt += [(a, p), (p, b)]
        frontier = nxt
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("variant", [0, 1, 2])
@pytest.mark.parametrize("leaf", [1, 4])
def test_centroids_exactly_on_planes(miro, variant, leaf):
    """Point triangles (a = b = c: the centroid is the point) at the fp32 planes the root's bisection on x visits in steps 0, 1
    and 2 for a box symmetric about 0: an object on the plane stays on its side (the move predicates are strict) while the
    final partition sends it right.  The rest are spread unevenly so that both sides are the heavy one in turn."""
    rng = np.random.default_rng(4200 + variant)
    half = F([4.0, 3.0, 10.0][variant])
    eps = F(1e-4)
    planes = bisection_planes(F(-half - eps), F(half + eps), 3)        # the padded root box on x
    assert planes[0] == 0 and len(planes) == 15
    xs = [-half, half]                                                   # the box's extremes
    for p in planes:
        xs += [p] * int(rng.integers(1, 4))
    dense = [(-half, F(0)), (F(0), half), (-half, half)][variant]        # where most of the others lie
    xs += list((rng.random(120) * (dense[1] - dense[0]) + dense[0]).astype(F))
    xs += list((rng.random(40) * 2 * half - half).astype(F))
    xs = np.asarray(xs, F)
    yz = (rng.integers(-4, 5, (len(xs), 2)) * 0.5).astype(F)            # a coarse grid: ties on the other axes too
    pts = np.concatenate([xs[:, None], yz], 1)
    pts = pts[rng.permutation(len(pts))]
    v = np.repeat(pts, 3, axis=0)
    f = np.arange(len(v), dtype=np.uint32).reshape(-1, 3)
    host, dev = both_builders(miro, mesh_filler(v, f), leaf)
    same_tree(host, dev)
    corners, _, _ = dev.export_tree()
    assert corners[0, 0] == F(-half - eps) and corners[0, 3] == F(half + eps)


@pytest.mark.gpu
def test_rebuild_host_device_host(miro):
    s = miro.Scene()
    scenes.populate(s, "teapot")
    trees = []
    for builder in (HOST, DEVICE, HOST):
        s.build(4, builder=builder)
        assert s.build_timing()["builder"] == builder
        i = s.info()
        trees.append((s.export_tree(), (i.n_nodes, i.n_leaves, i.max_depth)))
    for (c, m, p), i in trees[1:]:
        (c0, m0, p0), i0 = trees[0]
        assert i == i0 and np.array_equal(c.view(np.uint32), c0.view(np.uint32)) and np.array_equal(m, m0) and np.array_equal(p, p0)


@pytest.mark.gpu
def test_trace_after_a_device_build(miro):
    host, dev = miro.Scene(), miro.Scene()
    for s, builder in ((host, HOST), (dev, DEVICE)):
        scenes.populate(s, "teapot")
        s.build(4, builder=builder)
    assert dev.build_timing()["builder"] == DEVICE
    rays = random_rays(miro.RAY_DTYPE, 4096, [-4, -1, -4], [4, 4, 4], 168)
    want, got = host.trace(rays), dev.trace(rays)
    assert (want["prim"] != miro.MISS).sum() > 100
    assert got.tobytes() == want.tobytes()


@pytest.mark.gpu
@pytest.mark.parametrize("bad", [np.nan, np.inf])
def test_non_finite_input_is_built_on_the_host(miro, bad):
    """The scene calls accept a non-finite vertex; the object-table kernel finds it and the call builds on the host: MR_OK, the
    host's tree, builder_used = 0."""
    rng = np.random.default_rng(77)
    v = (rng.random((150, 3)) * 4 - 2).astype(F)
    v[31, 1] = bad
    f = np.arange(150, dtype=np.uint32).reshape(-1, 3)
    host, dev = both_builders(miro, mesh_filler(v, f), 2, finite=False)
    same_tree(host, dev)
