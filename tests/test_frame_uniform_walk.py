"""The uniform walk of the fused frame kernel (mr_traverse.h: uniform_run): a run whose lanes are all
the lanes of the wave that still have work goes on through leaves and pops -- the uniform leaf loop in place, every lane popping
its own stack, one comparison of the popped values -- instead of ending there.  No floating-point instruction, operand or order
of a lane's steps changes, so primary records, shadow records and pixels of the fused frame must be the batched pipeline's (which
takes no run) and the oracle's, byte for byte.

That a case reaches the path it is about is asserted on the CPU: replay_walks replays the whole walk of every wave of primary
rays in float32 on the exported tree -- node visits, the triangle tests of the leaves (float32 numpy division is the IEEE
division), every lane's stack, and the kernel's control flow at wave level (traverse's node loop and leaf step, node_step's
uniformity test, the run with its rule for leaves and pops).  The counts describe that model of the control flow, not the
kernel's own: what ties the two together is the source (the replay is written from uniform_run / uniform_walk / node_step / traverse)
and the replay's hit per ray, which must be the kernel's record -- a replay whose arithmetic or visiting order differed from the
kernel's would fail there; one that only grouped the lanes differently would not.  Eye rays are replayed in every case, the
closest-hit shadow rays (in the waves' lane order) where a case is about them; any-hit walks are covered by the byte-for-byte
comparison alone."""
import numpy as np
import pytest
import torch

from helpers import product_scene
from miro_amd import frame as mframe
from miro_amd import scenes

pytestmark = pytest.mark.gpu

DONE = -1
VIEWS = {
    "teapot": dict(lookat=(1.6, 1.0, 0.0), fov=10.0),         # the spout / body edge against the floor triangle
}


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32).numpy()


def _desc(name, **over):
    d = dict(scenes.SCENES[name]) if isinstance(name, str) else dict(name)
    if isinstance(name, str):
        d.update(VIEWS.get(name, {}))
    d.update(over)
    for k in ("eye", "lookat", "light"):
        d[k] = tuple(float(np.float32(v)) for v in d[k])
    return d


def _scene_of(miro, d, leaf_size=4):
    sc = miro.Scene(0)
    scenes.populate(sc, d)
    sc.build(leaf_size)
    return sc


def _regular_dir(d):
    ad = np.abs(d)
    return ((ad >= 2.0 ** -40) & (ad <= 2.0 ** 40)).all(axis=1)


def _regular_pos(o):
    ao = np.abs(o)
    return ((ao == 0) | ((ao >= 2.0 ** -36) & (ao <= 2.0 ** 60))).all(axis=1)


def _irregular_box(c):
    a = np.abs(c)
    return bool((~np.isfinite(c) | ((a != 0) & ((a < 2.0 ** -36) | (a > 2.0 ** 60)))).any())


def _pattern_distance(a, b):
    return np.abs(a.view(np.uint32).astype(np.int64) - b.view(np.uint32).astype(np.int64))


def triangle_records(sc):
    """A, B - A, C - A and their cross product per leaf-order position, rounded as mr_api.cpp rounds them"""
    v, _, vi, _ = sc.arrays()
    _, _, prims = sc.export_tree()
    f = np.float32
    A, B, C = (v[vi[prims, k]].astype(f) for k in range(3))
    e1, e2 = B - A, C - A
    n = np.stack([e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1], e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2],
                  e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]], 1).astype(f)
    return A, e1, e2, n


COUNTS = ("waves", "root_none", "root_partial", "dead_lanes", "walks", "subset_walks", "visits", "leaves", "empty_leaves", "long_leaves", "leaf_then_leaf",
          "leaf_then_node", "pops_agree", "pops_differ", "pops_differ_done", "walks_done", "irregular", "irregular_after_pop",
          "ties", "ties_after_leaf", "splits", "ends_at_leaf", "ends_at_pop")


def replay_walks(corners, meta, tris, rays, n_waves=None):
    """Every 64-ray wave of eye rays from the root test to its last pop.  Returns (counts, best position per ray, -1 = miss).
    A reference is an index into the exported tree (inner node or leaf), DONE when the lane's stack is empty.  Decisions are
    taken from the correctly rounded quotients: the guard of node_slabs_guarded makes the kernel's decisions exactly those
    (the products are computed too, to count the visits at which the wave recomputes).  A wave that would not take an octant
    loop of the run walk (mixed octants, an irregular direction) is walked lane by lane and counts nothing."""
    f = np.float32
    A, E1, E2, N = tris
    c = dict.fromkeys(COUNTS, 0)
    n = len(rays)
    waves = (n + 63) // 64 if n_waves is None else n_waves
    best_pos = np.full(waves * 64, -1, np.int64)
    from_walk = np.zeros(waves * 64, bool)             # the ray's hit was accepted by a leaf taken INSIDE a walk
    kEps = f(1e-4)
    one_eps = f(1) + kEps
    with np.errstate(all="ignore"):
        for w in range(waves):
            lo, hi = 64 * w, min(64 * w + 64, n)
            live = np.zeros(64, bool)
            live[:hi - lo] = rays["tmax"][lo:hi] >= 0        # (a wave-ordered shadow batch marks the lanes without a ray with tMax = -1)
            o = np.zeros((64, 3), f)
            d = np.ones((64, 3), f)
            tmax = np.full(64, -1, f)
            r = rays[lo:hi]
            o[:hi - lo] = np.stack([r["ox"], r["oy"], r["oz"]], 1)
            d[:hi - lo] = np.stack([r["dx"], r["dy"], r["dz"]], 1)
            tmax[:hi - lo] = r["tmax"]
            inv = f(1.0) / d
            md = -d
            c["waves"] += 1
            c["dead_lanes"] += int(not live.all())
            if not live.any():
                continue
            neg = d < 0
            # (eye rays are traced on the eye-relative tables from a zero origin: an irregular eye does not keep the wave out of the
            # octant loops, it marks every node irregular)
            run_walk = bool((neg[live] == neg[live][0]).all() and _regular_dir(d[live]).all() and (r["tmin"][live[:hi - lo]] == 0).all())
            eye_irregular = not _regular_pos(o[live]).all()
            oct_neg = neg[live][0]

            def slabs(box, exact):
                near = np.where(oct_neg, box[3:], box[:3]).astype(f) if run_walk else None
                if not run_walk:                       # generic form: min / max of both corners per axis
                    a, b = (box[:3] - o) / d, (box[3:] - o) / d
                    return np.minimum(a, b).max(axis=1), np.maximum(a, b).min(axis=1)
                far = np.where(oct_neg, box[:3], box[3:]).astype(f)
                if exact:
                    return ((near - o) / d).max(axis=1), ((far - o) / d).min(axis=1)
                return ((near - o) * inv).max(axis=1), ((far - o) * inv).min(axis=1)

            best = tmax.copy()
            pos = np.full(64, -1, np.int64)
            in_walk = np.zeros(64, bool)
            stack = [[DONE] for _ in range(64)]
            mn, mx = slabs(corners[0], True)
            root = live & ~((mn > mx) | (mn > tmax) | (mx < 0))
            cur = np.where(root, 0, DONE)
            if not root.any():
                c["root_none"] += 1
            elif not root[live].all():
                c["root_partial"] += 1

            def decide(node, lanes):
                """node_decide for `lanes` (a bool mask) at inner node `node`: returns h0, h1, first1 and whether the wave recomputes"""
                c0, c1 = int(meta[node, 1]), int(meta[node, 2])
                mn0, mx0 = slabs(corners[c0], True)
                mn1, mx1 = slabs(corners[c1], True)
                h0 = ~((mn0 > np.minimum(mx0, best)) | (mx0 < 0))
                h1 = ~((mn1 > np.minimum(mx1, best)) | (mx1 < 0))
                tie = False
                if run_walk:
                    p0, q0 = slabs(corners[c0], False)
                    p1, q1 = slabs(corners[c1], False)
                    k0, k1 = np.minimum(q0, best), np.minimum(q1, best)
                    close = np.zeros(64, bool)
                    for a, b in ((p0, k0), (p1, k1), (p0, p1)):
                        close |= (_pattern_distance(a, b) <= 16) & (a != 0) & (b != 0)
                    tie = bool((close & lanes).any())
                return c0, c1, h0, h1, mn0 > mn1, tie

            def lane_visit(lanes):
                for node in np.unique(cur[lanes]):
                    at = lanes & (cur == node)
                    c0, c1, h0, h1, first1, _ = decide(int(node), at)
                    for i in np.nonzero(at)[0]:
                        if h0[i] and h1[i]:
                            near, far = (c1, c0) if first1[i] else (c0, c1)
                            stack[i].append(far)
                            cur[i] = near
                        elif h0[i] or h1[i]:
                            cur[i] = c0 if h0[i] else c1
                        else:
                            cur[i] = stack[i].pop()

            def leaf(node, lanes, walking=False):
                first, cnt = int(meta[node, 1]), int(meta[node, 2])
                for k in range(first, first + cnt):
                    p = o - A[k]
                    ddotn = (md[:, 0] * N[k, 0] + md[:, 1] * N[k, 1]) + md[:, 2] * N[k, 2]
                    t = ((p[:, 0] * N[k, 0] + p[:, 1] * N[k, 1]) + p[:, 2] * N[k, 2]) / ddotn
                    ux = p[:, 1] * E2[k, 2] - p[:, 2] * E2[k, 1]
                    uy = p[:, 2] * E2[k, 0] - p[:, 0] * E2[k, 2]
                    uz = p[:, 0] * E2[k, 1] - p[:, 1] * E2[k, 0]
                    beta = ((md[:, 0] * ux + md[:, 1] * uy) + md[:, 2] * uz) / ddotn
                    wx = E1[k, 1] * p[:, 2] - E1[k, 2] * p[:, 1]
                    wy = E1[k, 2] * p[:, 0] - E1[k, 0] * p[:, 2]
                    wz = E1[k, 0] * p[:, 1] - E1[k, 1] * p[:, 0]
                    gamma = ((md[:, 0] * wx + md[:, 1] * wy) + md[:, 2] * wz) / ddotn
                    reject = (beta < -kEps) | (gamma < -kEps) | (beta + gamma > one_eps) | (t < 0) | (t > best)
                    take = lanes & ~reject & (t < best)
                    best[take] = t[take]
                    pos[take] = k
                    in_walk[take] = walking

            def walk(node, lanes, whole):
                """uniform_run from inner node `node` with the lanes `lanes`; leaves the lanes' cur as the kernel leaves L.cur"""
                c["walks"] += 1
                c["subset_walks"] += int(not whole)
                popped = had_leaf = False
                after_leaf = False                     # the step before this one was a leaf and its pop
                while True:
                    c["visits"] += 1
                    c0, c1 = int(meta[node, 1]), int(meta[node, 2])
                    if after_leaf:
                        c["leaf_then_node"] += 1
                    after_leaf = False
                    if eye_irregular or _irregular_box(corners[c0]) or _irregular_box(corners[c1]):
                        c["irregular"] += 1
                        c["irregular_after_pop"] += int(popped)
                        cur[lanes] = node
                        lane_visit(lanes)
                        return
                    _, _, h0, h1, first1, tie = decide(node, lanes)
                    c["ties"] += int(tie)
                    c["ties_after_leaf"] += int(tie and had_leaf)
                    a0, a1, f1 = h0[lanes], h1[lanes], first1[lanes]
                    pop = False
                    if a0.all() and a1.all() and (f1.all() or not f1.any()):
                        near, far = (c1, c0) if f1.all() else (c0, c1)
                        for i in np.nonzero(lanes)[0]:
                            stack[i].append(far)
                        nxt = near
                    elif a0.all() and not a1.any():
                        nxt = c0
                    elif a1.all() and not a0.any():
                        nxt = c1
                    elif not a0.any() and not a1.any() and whole:
                        pop = True
                    else:                              # a split decision, or a pop a subset may not take: lane by lane
                        c["splits" if (a0 | a1).any() else "ends_at_pop"] += 1
                        cur[lanes] = node
                        lane_visit(lanes)
                        return
                    while True:
                        if pop:
                            vals = [stack[i].pop() for i in np.nonzero(lanes)[0]]
                            popped = True
                            if len(set(vals)) > 1:
                                c["pops_differ"] += 1
                                c["pops_differ_done"] += int(DONE in vals)
                                cur[np.nonzero(lanes)[0]] = vals
                                return
                            c["pops_agree"] += 1
                            nxt = vals[0]
                            if nxt == DONE:
                                c["walks_done"] += 1
                                cur[lanes] = DONE
                                return
                        if not meta[nxt, 0]:
                            node = nxt
                            break
                        if not whole:                  # the others wait at their leaves: the wave's leaf step takes this one
                            c["ends_at_leaf"] += 1
                            cur[lanes] = nxt
                            return
                        c["leaves"] += 1
                        c["empty_leaves"] += int(meta[nxt, 2] == 0)
                        c["long_leaves"] += int(meta[nxt, 2] >= 15)
                        c["leaf_then_leaf"] += int(after_leaf)
                        leaf(nxt, lanes, True)
                        had_leaf = after_leaf = pop = True

            # traverse, while-while
            while (cur != DONE).any():
                have = cur != DONE
                while True:
                    at_node = have & (cur != DONE)
                    at_node[at_node] = meta[cur[at_node], 0] == 0
                    if not at_node.any():
                        break
                    first = cur[at_node][0]
                    if run_walk and (cur[at_node] == first).all():
                        walk(int(first), at_node, bool((at_node == have).all()))
                        at_node &= cur != DONE
                        at_node[at_node] = meta[cur[at_node], 0] == 0
                    if at_node.any():
                        lane_visit(at_node)
                at_leaf = cur != DONE
                for node in np.unique(cur[at_leaf]):
                    leaf(int(node), at_leaf & (cur == node))
                for i in np.nonzero(at_leaf)[0]:
                    cur[i] = stack[i].pop()
            best_pos[lo:lo + 64] = pos
            from_walk[lo:lo + 64] = in_walk
    if n_waves is None:
        return c, best_pos[:n], from_walk[:n]
    return c, best_pos, from_walk


def _render(miro, oracle, d, W, H, spp, sc=None, tiled=False, any_shadow=False, no_shadows=False, with_oracle=True, leaf_size=4):
    """the fused frame against the batched pipeline and, on the batched pipeline's rays, against the oracle"""
    if sc is None:
        sc = _scene_of(miro, d, leaf_size)
    ref = mframe.FrameRenderer(sc, d, W, H, spp=spp, tiled=tiled)
    ref.generate()
    if no_shadows:                       # no shadow ray is traced, every hit is lit: the batched shade given misses
        ref.trace_primary()
        ref.make_shadow_rays()
        ref.d_shadow_hits.zero_()
        ref.d_shadow_hits.view(torch.int32)[:, 1] = -1
        ref.shade()
    else:
        ref.step(any_hit=any_shadow)
    fu = mframe.FusedFrame(sc, d, W, H, spp=spp, tiled=tiled, keep_hits=True, any_shadow=any_shadow, no_shadows=no_shadows)
    fu.step()
    torch.cuda.synchronize()
    assert np.array_equal(_bits(fu.d_hits), _bits(ref.d_hits))
    src = None
    if no_shadows:
        assert fu.ray_counts() == (ref.n, 0)
    else:
        n_p, n_s = ref.ray_counts()
        assert fu.ray_counts() == (n_p, n_s)
        src = ref.d_src[:n_s].to(torch.int64)
        assert np.array_equal(_bits(fu.d_shadow_hits[src]), _bits(ref.d_shadow_hits[:n_s]))
    assert np.array_equal(_bits(fu.d_rgb), _bits(ref.d_rgb))
    rays = np.frombuffer(ref.d_rays.cpu().numpy().tobytes(), dtype=oracle.RAY_DTYPE)
    if with_oracle:
        osc = oracle.Scene()
        scenes.populate(osc, d)
        osc.build(leaf_size)
        assert fu.d_hits.cpu().numpy().tobytes() == osc.trace(rays).tobytes(), "primary records differ from the oracle"
        if src is not None and len(src) and not any_shadow:
            srays = np.frombuffer(ref.d_shadow_rays[:len(src)].cpu().numpy().tobytes(), dtype=oracle.RAY_DTYPE)
            assert fu.d_shadow_hits[src].cpu().numpy().tobytes() == osc.trace(srays).tobytes(), "shadow records differ from the oracle"
    return sc, fu, ref, rays, src


def _replay(miro, sc, fu, rays, n_waves=None, hits=None, with_walk_hits=False):
    """replay_walks on the frame's eye rays (or on `rays` against the records `hits`); the replay's hit per ray must be the kernel's"""
    corners, meta, prims = sc.export_tree()
    counts, pos, from_walk = replay_walks(corners, meta, triangle_records(sc), rays if n_waves is None else rays[:64 * n_waves])
    hits = fu.d_hits if hits is None else hits
    prim = hits.cpu().numpy().view(miro.HIT_DTYPE).reshape(-1)["prim"][:len(pos)]
    want = np.where(pos >= 0, prims[np.maximum(pos, 0)], np.uint32(0xFFFFFFFF)).astype(np.uint32)
    assert np.array_equal(prim, want), "the replay's hits are not the kernel's"
    return (counts, pos, from_walk) if with_walk_hits else counts


def _shadow_waves(ref, src, n):
    """the shadow rays in the lane order of the fused frame's waves: sample i's ray at index i, tMax = -1 where there is none"""
    rays = np.zeros(n, dtype=np.dtype([("ox", "<f4"), ("oy", "<f4"), ("oz", "<f4"), ("tmin", "<f4"),
                                       ("dx", "<f4"), ("dy", "<f4"), ("dz", "<f4"), ("tmax", "<f4")]))
    rays["dx"] = rays["dy"] = rays["dz"] = 1.0
    rays["tmax"] = -1.0
    made = np.frombuffer(ref.d_shadow_rays[:len(src)].cpu().numpy().tobytes(), dtype=rays.dtype)
    rays[src.cpu().numpy()] = made
    return rays


@pytest.mark.parametrize("name", ["sponza", "teapot"])
def test_long_walks_one_pixel_per_wave(miro, oracle, name):
    # 16 x 8 at 64 samples per pixel in image order (the 128-lane build): a wave is one pixel
    sc, fu, _, rays, _ = _render(miro, oracle, _desc(name), 16, 8, 64)
    c = _replay(miro, sc, fu, rays)
    assert c["leaves"] > 0 and c["pops_agree"] > 0 and c["leaf_then_node"] > 0 and c["leaf_then_leaf"] > 0, str(c)
    assert c["walks_done"] > 0, str(c)                          # every lane pops its sentinel in one pop: the kDone exit
    assert c["pops_differ"] > 0 and c["splits"] > 0, str(c)     # lanes that parted and met again hold different stacks
    if name == "sponza":                                        # ... and in some of those pops lanes finish while others go on
        assert c["pops_differ_done"] > 0, str(c)


@pytest.mark.parametrize("name", ["sponza", "teapot"])
@pytest.mark.parametrize("spp", [4, 1])
def test_tiled_waves_fall_back(miro, oracle, name, spp):
    # 64 x 36 in the tiled order: a wave is a tile of 4 x 4 or 8 x 8 pixels; runs of a subset of the working lanes end at leaves
    # and pops as they always did, and whole walks meet pops whose values differ
    sc, fu, _, rays, _ = _render(miro, oracle, _desc(name), 64, 36, spp, tiled=True)
    c = _replay(miro, sc, fu, rays)
    assert c["subset_walks"] > 0 and c["ends_at_leaf"] + c["ends_at_pop"] > 0 and c["pops_differ"] > 0, str(c)


@pytest.mark.parametrize("name", ["sponza", "teapot"])
def test_256_lane_launch(miro, oracle, name):
    # 625 x 256 x 64: the smallest frame of test_frame_large.py that takes the 256-lane build; the first 128 waves are replayed
    sc, fu, _, rays, _ = _render(miro, oracle, _desc(name), 625, 256, 64, sc=product_scene(miro, name), with_oracle=False)
    assert fu.n > 10000000
    c = _replay(miro, sc, fu, rays, n_waves=128)
    assert c["leaves"] > 0 and c["pops_agree"] > 0, str(c)


def test_extended_count_leaves_and_the_last_record_inside_walks(miro, oracle):
    # The atrium built with leaves of up to 16 triangles: leaves of 15 and more keep their count in leaf_cnt_ext, and here their
    # parents are ordinary nodes, so walks take them in place.  The camera aims at the triangle whose record is the table's last:
    # camera rays and shadow rays report it from leaves taken inside walks.
    d = _desc("sponza")
    probe = _scene_of(miro, d, 16)
    v, _, vi, _ = probe.arrays()
    _, meta, prims = probe.export_tree()
    target = v[vi[int(prims[-1])]].mean(axis=0)
    d = _desc("sponza", lookat=tuple(float(x) for x in target), fov=4.0)
    sc, fu, ref, rays, src = _render(miro, oracle, d, 16, 8, 64, sc=probe, leaf_size=16)
    leaves = meta[meta[:, 0] != 0]
    assert leaves[:, 2].max() >= 15 and int((leaves[:, 1] + leaves[:, 2]).max()) == len(prims)
    last = len(prims) - 1
    c, pos, from_walk = _replay(miro, sc, fu, rays, with_walk_hits=True)
    assert c["long_leaves"] > 0, str(c)
    assert ((pos == last) & from_walk).any(), "no camera ray takes the last record inside a walk"
    srays = _shadow_waves(ref, src, fu.n)
    cs, spos, sfrom = _replay(miro, sc, fu, srays, hits=fu.d_shadow_hits, with_walk_hits=True)
    # (no shadow ray of this view meets the last triangle -- the rays start on it; the cards below have shadow rays report the last
    # record.  Here: the shadow walks take leaves, extended ones among them, and their hits come from those leaves.)
    assert cs["leaves"] > 0 and cs["long_leaves"] > 0 and cs["pops_agree"] > 0, str(cs)
    assert ((spos >= 0) & sfrom).any(), "no shadow ray takes its hit inside a walk"


# ---- leaf shapes: test_frame_scalar_side.py's row of cards, tilted 45 degrees about y, cut into 1 .. 4 triangles or 16 times the same one
CARDS = (4, 1, 4, 2, 4, 3, 16, 4, 2, 16, 1, 4)


def _card(cx, n):
    h = 0.5
    s = np.float32(np.sqrt(0.5))

    def at(u, v):
        return (float(cx + u * h * s), float(v * h), float(-u * h * s))
    nrm = (float(s), 0.0, float(s)) * 3
    if n == 16:
        return [("triangle", at(-1, -1) + at(1, -1) + at(0, 1), nrm)] * 16
    if n == 1:
        return [("triangle", at(-1, -1) + at(1, -1) + at(0, 1), nrm)]
    t = np.linspace(0.0, 2.0, n + 1)
    rim = [(1.0, min(1.0, -1.0 + 2.0 * x)) if x <= 1.0 else (1.0 - 2.0 * (x - 1.0), 1.0) for x in t]
    return [("triangle", at(-1, -1) + at(*rim[i]) + at(*rim[i + 1]), nrm) for i in range(n)]


def cards_desc(**over):
    objs = []
    for k, n in enumerate(CARDS):
        objs += _card(1.5 * k, n)
    span = 1.5 * (len(CARDS) - 1)
    d = dict(models=[], floor=None, objects=objs, eye=(span / 2, 0.0, 9.0), lookat=(span / 2, 0.0, 0.0), up=scenes.UP, fov=15.0,
             light=(span + 40.0, 0.0, 0.0), wattage=4000.0)
    d.update(over)
    return _desc(d)


def test_leaf_shapes_inside_walks(miro, oracle):
    d = cards_desc()
    sc, fu, _, rays, src = _render(miro, oracle, d, 48, 6, 64)
    _, meta, prims = sc.export_tree()
    leaves = meta[meta[:, 0] != 0]
    first, count = leaves[:, 1], leaves[:, 2]
    assert {0, 1, 2, 3, 4, 16} <= set(count.tolist()), sorted(set(count.tolist()))
    assert int((first + count).max()) == len(prims)                        # the last leaf ends at the table's end
    last = int(prims[-1])
    prim = fu.d_hits.cpu().numpy().view(miro.HIT_DTYPE).reshape(-1)["prim"]
    sprim = fu.d_shadow_hits[src].cpu().numpy().view(miro.HIT_DTYPE).reshape(-1)["prim"]
    assert (prim == last).any(), "no camera ray reports the last record"
    assert (sprim == last).any(), "no shadow ray reports the last record"
    big = np.nonzero(count >= 15)[0]                                       # the extended-count leaves are hit by both
    in_big = np.concatenate([prims[first[i]:first[i] + count[i]] for i in big])
    assert np.isin(prim, in_big).any() and np.isin(sprim, in_big).any()
    c = _replay(miro, sc, fu, rays)
    assert c["leaves"] > 0, str(c)
    # An empty leaf keeps the empty box (lo = +inf, hi = -inf): no ray enters it, in a walk or out of one, and the node above it is an
    # irregular one -- the walk that meets it leaves for the true divisions.  58 of the tree's 69 inner nodes are such.
    empty = np.nonzero((meta[:, 0] != 0) & (meta[:, 2] == 0))[0]
    corners, _, _ = sc.export_tree()
    assert len(empty) > 0 and np.isinf(corners[empty]).all()
    assert c["empty_leaves"] == 0 and c["irregular"] > 0, str(c)
    # (This scene's leaves of 16 hang below chains of such nodes -- the builder peels empty halves off them down to depth 32 -- and
    # are reached through leaf_step; test_extended_count_leaves_and_the_last_record_inside_walks has the walk read the extended count.)


def test_ragged_last_wave(miro, oracle):
    # 13 x 7 pixels x 16 samples = 1 456 samples: the last wave has 48 live lanes, dead ones from the start
    sc, fu, _, rays, _ = _render(miro, oracle, _desc("teapot"), 13, 7, 16)
    c = _replay(miro, sc, fu, rays)
    assert c["dead_lanes"] == 1 and c["leaves"] > 0, str(c)


def test_part_of_a_wave_misses_the_root_box(miro, oracle):
    # the camera aims at a corner of the root box from far away: pixels there have samples inside and outside its outline
    d = cards_desc()
    corners, _, _ = _scene_of(miro, d).export_tree()
    hi = corners[0][3:]
    d = cards_desc(eye=(float(hi[0]) + 2.0, float(hi[1]) + 3.0, 40.0), lookat=(float(hi[0]), float(hi[1]), float(corners[0][2])), fov=1.0)
    sc, fu, _, rays, _ = _render(miro, oracle, d, 16, 8, 64)
    c = _replay(miro, sc, fu, rays)
    assert c["root_partial"] > 0 and c["walks"] > 0, str(c)


def test_background_only(miro, oracle):
    # the camera looks away from the scene: the root test fails in every lane and no walk is entered
    d = cards_desc(lookat=(8.25, 0.0, 20.0))
    sc, fu, _, rays, _ = _render(miro, oracle, d, 16, 8, 64)
    c = _replay(miro, sc, fu, rays)
    assert c["root_none"] == c["waves"] == 128 and c["walks"] == 0, str(c)
    assert (fu.d_hits[:, 1].view(torch.int32) == -1).all()


def test_irregular_node_after_a_pop(miro, oracle):
    # A triangle whose lowest corner sits one ulp above the boxes' padding (1e-4): its leaf's padded box has a corner of 2^-37,
    # below what the correction steps may divide -- an irregular node deep in the tree, next to the teapot, which walks reach
    # after their first leaves and pops.  (A triangle with corners beyond 2^60 makes the ROOT's visit irregular: every walk
    # would leave at its first visit.)
    low = float(np.nextafter(np.float32(1e-4), np.float32(1)))
    wall = ("triangle", (1.2, low, 0.5, 2.0, low, 0.5, 1.6, 1.5, 0.5), (0, 0, 1) * 3)
    d = _desc("teapot", objects=[wall])
    sc, fu, _, rays, _ = _render(miro, oracle, d, 16, 8, 64)
    c = _replay(miro, sc, fu, rays)
    assert c["irregular"] > 0 and c["irregular_after_pop"] > 0, str(c)


def test_irregular_eye(miro, oracle):
    # one eye component below 2^-36: the eye-relative tables mark every node irregular -- every walk leaves at its first visit
    eye = list(scenes.SCENES["teapot"]["eye"])
    eye[0] = 1e-12
    sc, fu, _, rays, _ = _render(miro, oracle, _desc("teapot", eye=eye), 16, 8, 64)
    assert not _regular_pos(np.stack([rays["ox"], rays["oy"], rays["oz"]], 1)).any()
    c = _replay(miro, sc, fu, rays)
    assert c["walks"] > 0 and c["walks"] == c["visits"] == c["irregular"] and c["leaves"] == 0, str(c)


def test_near_tie_after_a_leaf(miro, oracle):
    # a wall of the Cornell box at grazing incidence: slab distances tie there, the wave recomputes the visit with exact
    # quotients -- here in walks that have already been through a leaf, with best_t below the rays' own tMax
    d = _desc("cornell", eye=(0.02, 2.5, 3.0), lookat=(0.0, 2.5, -2.0), fov=20.0)
    sc, fu, _, rays, _ = _render(miro, oracle, d, 16, 8, 64)
    c = _replay(miro, sc, fu, rays)
    assert c["ties"] > 0 and c["ties_after_leaf"] > 0, str(c)


@pytest.mark.parametrize("mode", ["any_shadow", "no_shadows"])
def test_shadow_forms(miro, oracle, mode):
    # any-hit shadow rays (their walks take the pops and end at every leaf: byte for byte only, the replay is of the eye rays) and the
    # launch without shadow rays
    sc, fu, _, rays, _ = _render(miro, oracle, _desc("sponza"), 16, 8, 64, any_shadow=mode == "any_shadow", no_shadows=mode == "no_shadows")
    c = _replay(miro, sc, fu, rays)
    assert c["leaves"] > 0 and c["pops_agree"] > 0, str(c)


def test_per_object_materials_take_no_run(miro):
    # a scene with a material table is shaded per object (the MAT kernels): no run, no walk.  The batched shade refuses such a
    # scene, so the records are compared with the batched traces.
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


def test_captured_frame_replayed_twice(miro, oracle):
    d = _desc("sponza")
    sc, _, ref, _, src = _render(miro, oracle, d, 16, 8, 64)     # ref: the batched pipeline
    fu = mframe.FusedFrame(sc, d, 16, 8, spp=64, tiled=False, keep_hits=True)
    fu.step()                                   # the eye tables of this camera exist before the capture
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        fu.step(stream=side)
    for _ in range(2):
        fu.d_rgb.fill_(-1.0)
        fu.d_hits.view(torch.int32).fill_(0x7FC0BEEF)
        fu.d_shadow_hits.view(torch.int32).fill_(0x7FC0BEEF)
        g.replay()
        torch.cuda.synchronize()
        assert np.array_equal(_bits(fu.d_rgb), _bits(ref.d_rgb))
        assert np.array_equal(_bits(fu.d_hits), _bits(ref.d_hits))
        assert np.array_equal(_bits(fu.d_shadow_hits[src]), _bits(ref.d_shadow_hits[:len(src)]))
