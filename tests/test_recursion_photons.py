"""mr_render_recursion_photons on the MI355X (include/miro_hip_recursion_photons.h, csrc/mr_gather_queued.hip): the one-call
recursive frame with the photon-map term of Scene::traceScene (Scene.cpp:286-299) after every level, by kernels that read the
length of the level's queue from the device.

The yardstick of every comparison is render_specular(fused="frame_lights" | "frame_lights_path", photon_maps=...) with tiled=False
and the same maps and arguments: existing code, whose level 0 is the same launch followed by mr_gather_level on generate()'s eye
rays, and whose further levels are mr_trace_level_lights[_path] + mr_gather_level with every length read back to the host.  A
FrameRenderer subclass keeps what that route computes on its way -- the six counters of every level, the d_counts of every
mr_gather_level and the pixel column of every queue.

Maps: Scene.photon_maps from a DirectionalAreaLight above the scene, a few thousand photons each, nphotons = 50, max_dist = 1e10.
Every case asserts that it gathered: the global map holds photons, level 0 has queries, and so has some level >= 1.

  counts   words 0..5 of every level EXACTLY the yardstick's, word 6 its query count of that level, word 7 zero; a level's children
           are the next level's rays
  pixels   rtol = 1e-5, atol = 1e-6 x max|rgb|, the bound tests/test_recursion_device.py and tests/test_level_lights.py hold
           float-atomic pixel sums to; bit for bit on the mirror-only scene at 1 spp, where no pixel occurs twice in a level (asserted
           from the yardstick's queues): per pixel both routes then do the same stores and adds in the same stream order, and the
           estimates do not depend on which wave pulls which batch (tests/test_gather_level.py finds them byte-equal between runs)"""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_frame_lights import bits, camera  # noqa: E402
from test_frame_level_lights import GLASS_DESC  # noqa: E402
from test_level_lights import ENVS, use  # noqa: E402
from test_recursion_device import DEPTH, GLASS_LIGHTS, MIRROR_ONLY, PATH, SEED, SPECULAR, WINDOWS  # noqa: E402
from test_recursion_device import scene as device_scene  # noqa: E402

K, MAX_DIST = 50, 1e10
TARGET = 3000                                           # photons per map
# a DirectionalAreaLight above each scene, facing down onto it (the flower and the stone room bring their own disc light)
DISCS = {"glass": dict(position=(0.5, 6.0, 0.0), normal=(0.0, -1.0, 0.0), color=(1.0, 1.0, 1.0), wattage=60.0, radius=2.5),
         "mirror": dict(position=(0.0, 7.0, 1.0), normal=(0.0, -1.0, 0.0), color=(1.0, 0.9, 0.8), wattage=80.0, radius=3.0),
         "teapot": dict(position=(0.0, 12.0, 0.0), normal=(0.0, -1.0, 0.0), color=(1.0, 1.0, 1.0), wattage=80.0, radius=4.0)}
_MAPS = {}
_GLASS = {}


def glass_room(miro):
    """tests/test_recursion_device.py's glass sphere (kd = 0, ks, kt = 0.9, index 1.5) and camera, over a diffuse floor and in front
    of a diffuse back wall: the sphere alone has no diffuse hit, so no photon is stored and nothing is gathered.  Here level 0
    sees floor and wall beside the sphere, and the Fresnel and refracted rays of the levels >= 1 reach them through it."""
    s = miro.Scene(0)
    s.add_triangle([-30, -1.2, 30, 30, -1.2, 30, 0, -1.2, -30], [0, 1, 0] * 3)
    s.add_triangle([-30, -1.2, -4, 30, -1.2, -4, 0, 40, -4], [0, 0, 1] * 3)
    s.add_sphere((0.0, 0.0, 0.0), 1.0)
    s.set_materials([((0.5, 0.5, 0.5), (0, 0, 0), (0, 0, 0), 1.0, 1.0), ((0.0, 0.0, 0.0), (0.05, 0.05, 0.05), (0.9, 0.9, 0.9), 80.0, 1.5)],
                    [0, 0, 1])
    s.build(4)
    return s


def scene(miro, name, env):
    """(scene, description, lights) with the lights and the environment ENVS[env] set: tests/test_recursion_device.py's scenes, the
    stone room of tests/test_level_lights.py, and the glass room above"""
    if name == "stone":
        return use(miro, name, env)
    if name != "glass":
        return device_scene(miro, name, env)
    if not _GLASS:
        _GLASS["s"] = glass_room(miro)
    s = _GLASS["s"]
    s.set_lights(GLASS_LIGHTS)
    s.set_environment(**(ENVS[env] or {}))
    return s, GLASS_DESC, GLASS_LIGHTS


def maps_of(miro, name, s, desc):
    """(global, caustic) of a scene, traced once per session; a caustic walk that stored nothing gives None"""
    if name not in _MAPS:
        textured = name in ("flower_drops", "stone")
        light = DISCS.get(name) or (desc["disc_light"] if name == "stone" else desc["lights"][0])
        if name == "teapot":                            # no specular material: a caustic walk would store nothing
            g, c = miro.PhotonMap(TARGET + 32), None
            s.trace_photons(g, light, TARGET, 4000000, resident=True)
        else:
            g, c = s.photon_maps(light, TARGET, 4000000, surface=textured)
        print(name, "photons", g.count(), c.count() if c is not None else None)
        assert g.count() >= TARGET                      # a case that gathered nothing proves nothing
        _MAPS[name] = (g, c if c is not None and c.count() > 0 else None)
    return _MAPS[name]


def pick(maps, which):
    g, c = maps
    return {"both": (g, c), "global": (g, None), "caustic": (None, c)}[which]


def frames(miro, name, env, children, spp, which="both", kinds=7, depth=DEPTH, capacity=None, window=None, plain=False):
    """The yardstick frame and the frame under test with the same arguments and maps.  Returns (ref, dev): each with per_level,
    rgb and counts; ref besides with queries (per level it ran) and pixels (the pixel column of every queue of levels >= 1).
    plain: both frames WITHOUT maps instead (fused="frame_lights[_path]" / "device_lights[_path]")."""
    import torch
    from miro_amd import frame

    class Spy(frame.FrameRenderer):
        def _level_buffers(self, plan, n, level, last):
            out = super()._level_buffers(plan, n, level, last)
            self.seen_counts.append(out[2])
            return out

        def _level_lights(self, plan, q, level, last, rgb=None):
            self.seen_pixels.append(q.pixels)
            return super()._level_lights(plan, q, level, last, rgb=rgb)

        def _gather(self, plan, q, hits, normal, rgb):
            """the route's own call, with mr_gather_level's optional d_counts ([0] queries, [1] rays) handed in besides"""
            real, spy = self.scene.gather_level, self

            def counted(*a, **kw):
                cnt = torch.zeros(2, dtype=torch.int64, device=spy.device)
                spy.seen_queries.append(cnt)
                return real(*a, d_counts=cnt, **kw)
            self.scene.gather_level = counted
            try:
                super()._gather(plan, q, hits, normal, rgb)
            finally:
                del self.scene.gather_level

    s, desc, lights = scene(miro, name, env)
    maps = None if plain else pick(maps_of(miro, name, s, desc), which)
    assert plain or any(m is not None for m in maps)
    w, h = window or WINDOWS[spp]
    kw = dict(depth=depth, lights=lights, environment=ENVS[env])
    if children == PATH:
        kw.update(path_tracing=True, path_kinds=kinds, path_seed=SEED)
    if not plain:
        kw.update(photon_maps=maps, nphotons=K, max_dist=MAX_DIST)
    route = "lights_path" if children == PATH else "lights"
    ref = Spy(s, desc, w, h, spp=spp, tiled=False)
    ref.seen_counts, ref.seen_pixels, ref.seen_queries = [], [], []
    ref.per_level = ref.render_specular(fused="frame_" + route, **kw)
    torch.cuda.synchronize()
    ref.counts = [c.tolist() for c in ref.seen_counts]
    ref.queries = [c.tolist() for c in ref.seen_queries]
    ref.pixels = [p.cpu().numpy() for p in ref.seen_pixels]
    ref.rgb = ref.d_rgb.clone()
    dev = frame.FrameRenderer(s, desc, w, h, spp=spp, tiled=False, resident_rays=False)
    dev.per_level = dev.render_specular(fused=("device_" + route) if plain else "device_photons" + route[len("lights"):],
                                        queue_capacity=capacity, **kw)
    torch.cuda.synchronize()
    dev.counts = dev.d_level_counts[:depth + 1].tolist()
    dev.rgb = dev.d_rgb.clone()
    return ref, dev


def assert_gathered(ref):
    """level 0 has queries, and so has some level >= 1; every mr_gather_level saw the level's rays"""
    assert len(ref.queries) == len(ref.counts)
    assert all(q[1] == c[0] for q, c in zip(ref.queries, ref.counts))
    assert ref.queries[0][0] > 0 and any(q[0] > 0 for q in ref.queries[1:]), ref.queries


def assert_counts(ref, dev, depth=DEPTH):
    """words 0..5 of every level the yardstick ran and word 6 = its queries there; the levels it did not run are all-zero rows;
    word 7 is 0; a level's children are the next level's rays"""
    assert len(dev.counts) == depth + 1 and all(len(row) == 8 for row in dev.counts)
    for level, row in enumerate(dev.counts):
        ran = level < len(ref.counts)
        want = ref.counts[level][:6] + [ref.queries[level][0]] if ran else [0] * 7
        assert row[:7] == want, (level, row, want)
        assert row[7] == 0
        if level < depth:
            assert dev.counts[level + 1][0] == row[5]
    assert dev.per_level == ref.per_level


def assert_pixels_close(got, want):
    import torch
    scale = float(want.abs().max())
    assert scale > 0
    assert torch.allclose(got, want, rtol=1e-5, atol=1e-6 * scale), float((got - want).abs().max())


@pytest.mark.gpu
@pytest.mark.parametrize("children", [SPECULAR, PATH], ids=["specular", "path"])
@pytest.mark.parametrize("spp", [1, 4])
@pytest.mark.parametrize("window", [(24, 16), (40, 24)], ids=["24x16", "40x24"])
@pytest.mark.parametrize("name", ["glass", "flower_drops", "mirror"])
def test_counts_exactly_and_pixels_within_the_atomic_bound(miro, name, window, spp, children):
    ref, dev = frames(miro, name, "colour", children, spp, window=window)
    print("per_level", ref.per_level, "counts", ref.counts, "queries", ref.queries)
    assert len(ref.per_level) == DEPTH + 1 and all(n > 0 for n, _ in ref.per_level)      # the case runs every level
    assert ref.counts[0][0] == window[0] * window[1] * spp and (spp > 1 or ref.counts[0][0] % 256 != 0)
    assert spp > 1 or any(row[5] % 256 != 0 for row in ref.counts[:DEPTH])
    assert_gathered(ref)
    assert_counts(ref, dev)
    assert_pixels_close(dev.rgb, ref.rgb)


@pytest.mark.gpu
@pytest.mark.parametrize("children", [SPECULAR, PATH], ids=["specular", "path"])
@pytest.mark.parametrize("which", ["global", "caustic"])
def test_one_map_alone(miro, which, children):
    """(global, None) and (None, caustic) on the glass sphere, whose caustic map is not empty (asserted)"""
    s, desc, _ = scene(miro, "glass", None)
    assert maps_of(miro, "glass", s, desc)[1] is not None
    ref, dev = frames(miro, "glass", None, children, 4, which=which)
    assert_gathered(ref)
    assert_counts(ref, dev)
    assert_pixels_close(dev.rgb, ref.rgb)


@pytest.mark.gpu
@pytest.mark.parametrize("children", [SPECULAR, PATH], ids=["specular", "path"])
def test_mirror_only_at_one_sample_is_the_yardsticks_bits(miro, children):
    """One ray per pixel and level: the precondition is asserted from the yardstick's own queues, then d_rgb is compared on its
    bits (level 0 is a store and one add, every further level two adds per pixel, all ordered by the stream)."""
    ref, dev = frames(miro, "mirror", "colour", children, 1, kinds=MIRROR_ONLY)
    assert len(ref.pixels) == DEPTH and len(ref.pixels[0]) > 256 and all(len(p) > 0 for p in ref.pixels)
    for level, p in enumerate(ref.pixels, 1):
        assert len(np.unique(p)) == len(p), level
    assert_gathered(ref)
    assert_counts(ref, dev)
    assert np.array_equal(bits(dev.rgb), bits(ref.rgb))


@pytest.mark.gpu
@pytest.mark.parametrize("name,children", [("glass", SPECULAR), ("flower_drops", PATH)])
def test_the_photon_term_is_there(miro, name, children):
    """the frame minus the same frame through fused="device_lights[_path]" is not zero, and is the yardstick's difference"""
    ref, dev = frames(miro, name, "colour", children, 4)
    ref0, dev0 = frames(miro, name, "colour", children, 4, plain=True)
    assert ref0.queries == [] and dev0.per_level == dev.per_level
    term, want = dev.rgb - dev0.rgb, ref.rgb - ref0.rgb
    print("photon term up to %.4g of %.4g" % (float(term.max()), float(ref.rgb.max())))
    assert float(want.abs().max()) > 1e-3 * float(ref.rgb.abs().max())
    import torch
    assert torch.allclose(term, want, rtol=1e-5, atol=1e-6 * float(ref.rgb.abs().max())), float((term - want).abs().max())


@pytest.mark.gpu
@pytest.mark.parametrize("children", [SPECULAR, PATH], ids=["specular", "path"])
def test_the_stone_room(miro, children):
    """the procedural room, whose queries take the bumped normal of the level's own normal buffer, at level 0 and beyond"""
    ref, dev = frames(miro, "stone", None, children, 4)
    print("per_level", ref.per_level, "queries", ref.queries)
    assert len(ref.per_level) == DEPTH + 1
    assert_gathered(ref)
    assert_counts(ref, dev)
    assert_pixels_close(dev.rgb, ref.rgb)


@pytest.mark.gpu
@pytest.mark.parametrize("spp", [1, 4])
def test_level_0_queries_are_the_batched_kernels_bits(miro, spp):
    """The level-0 query kernel against mr_gen_eye_rays + mr_trace + mr_hit_surface + mr_gather_level on the stone room, 40 x 24
    with jitter over rows [5, 19): positions and normals (a NaN normal where there is no query) through the scratch layout, which at
    depth 0 lies behind 16 n bytes of hit records and 12 n bytes of normals, each rounded up to 16 bytes."""
    import torch
    s, desc, lights = scene(miro, "stone", None)
    g, c = maps_of(miro, "stone", s, desc)
    w, h, y0, y1 = 40, 24, 5, 19
    n = (y1 - y0) * w * spp
    up = lambda v: (v + 15) // 16 * 16                                                                       # noqa: E731
    need = s.recursion_photons_workspace_bytes(camera(desc), w, h, 0, 0, y0=y0, y1=y1, spp=spp, children=0)
    assert need == up(16 * n) + up(12 * n) + up(48 * n)
    ws = torch.zeros(need, dtype=torch.uint8, device="cuda")
    rgb = torch.zeros(((y1 - y0) * w, 3), dtype=torch.float32, device="cuda")
    counts = torch.zeros((1, 8), dtype=torch.int64, device="cuda")
    s.render_recursion_photons(camera(desc), w, h, rgb, counts, 0, g, c, ws, max_dist=MAX_DIST, nphotons=K, y0=y0, y1=y1, spp=spp,
                               jitter=True, seed=SEED, children=0)
    rays = torch.empty((n, 8), dtype=torch.float32, device="cuda")
    hits = torch.empty((n, 4), dtype=torch.float32, device="cuda")
    color, normal = (torch.zeros((n, 3), dtype=torch.float32, device="cuda") for _ in range(2))
    scratch = torch.zeros(12 * n, dtype=torch.float32, device="cuda")
    term = torch.zeros((n, 3), dtype=torch.float32, device="cuda")
    cnt = torch.zeros(2, dtype=torch.int64, device="cuda")
    s.gen_eye_rays(camera(desc), w, h, rays, y0=y0, y1=y1, spp=spp, jitter=True, seed=SEED)
    s.trace_device(rays, n, hits)
    s.hit_surface(rays, hits, n, color, normal)
    s.gather_level(g, c, rays, hits, n, scratch, d_ray_rgb=term, d_normal=normal, max_dist=MAX_DIST, nphotons=K, spp=spp, d_counts=cnt)
    torch.cuda.synchronize()
    got = ws[up(16 * n) + up(12 * n):].view(torch.float32)[:6 * n].cpu().numpy().view(np.uint32)
    want = scratch[:6 * n].cpu().numpy().view(np.uint32)
    queries = int(cnt[0])
    assert queries > 100 and counts[0].tolist()[6] == queries and counts[0].tolist()[0] == n
    assert np.array_equal(got, want)
    nrm = scratch[3 * n:6 * n].view(n, 3).cpu().numpy()
    assert np.isfinite(nrm).all(axis=1).sum() == queries


@pytest.mark.gpu
@pytest.mark.parametrize("depth", [DEPTH, 0])
def test_a_queue_that_dies_out_and_depth_0(miro, depth):
    """The plain teapot has no specular material: with depth 3 the levels >= 1 are empty, and their gather launches (full grids,
    nq = 0) leave d_rgb and the counters as the yardstick has them.  Afterwards mr_irradiance_estimate on the same map answers, on
    each of the map's sixteen hand-out counters in turn, what it answered before the frame: the nq == 0 launches re-armed theirs.
    Rendering the frame twice gives equal counters."""
    import torch
    s, desc, lights = scene(miro, "teapot", None)
    g, _ = maps_of(miro, "teapot", s, desc)
    rng = np.random.default_rng(5)
    nq = 500
    pos = torch.from_numpy(rng.uniform(-3, 3, (nq, 3)).astype(np.float32)).cuda()
    nrm = torch.from_numpy(np.tile(np.float32([0, 1, 0]), (nq, 1))).cuda()

    def estimate():
        out = torch.full((nq, 3), -7.0, dtype=torch.float32, device="cuda")
        g.irradiance_estimate(pos, nrm, nq, out, max_dist=MAX_DIST, nphotons=K)
        torch.cuda.synchronize()
        return out.cpu().numpy()

    before = estimate()
    assert (before >= 0).all() and before.max() > 0
    ref, dev = frames(miro, "teapot", None, SPECULAR, 4, which="global", depth=depth)
    assert len(ref.per_level) == 1 and ref.queries[0][0] > 0
    assert_counts(ref, dev, depth)
    assert dev.counts[1:] == [[0] * 8] * depth
    assert_pixels_close(dev.rgb, ref.rgb)
    for _ in range(16):
        assert np.array_equal(estimate().view(np.uint32), before.view(np.uint32))
    _, again = frames(miro, "teapot", None, SPECULAR, 4, which="global", depth=depth)
    assert again.counts == dev.counts


@pytest.mark.gpu
def test_a_capacity_of_100_truncates_inside_the_declared_workspace(miro):
    """Level 0 of the glass sphere at 24 x 16 x 4 emits more than 100 children (asserted on the yardstick).  With queue_capacity =
    100 the call is MR_OK, [0][5] is the true count, level 1 runs exactly 100 rays, and the guard regions in front of and behind
    the declared workspace keep their pattern.  render_specular raises RuntimeError.  Once: a bounds check."""
    import torch
    from miro_amd import frame
    ref, _ = frames(miro, "glass", "colour", PATH, 4)
    true_children = ref.counts[0][5]
    assert true_children > 100
    s, desc, lights = scene(miro, "glass", "colour")
    g, c = maps_of(miro, "glass", s, desc)
    w, h = WINDOWS[4]
    need = s.recursion_photons_workspace_bytes(camera(desc), w, h, DEPTH, 100, spp=4, children=PATH, environment=True)
    guard = 4096
    buf = torch.full((guard + need + guard,), 0xA5, dtype=torch.uint8, device="cuda")
    rgb = torch.zeros((w * h, 3), dtype=torch.float32, device="cuda")
    counts = torch.zeros((DEPTH + 1, 8), dtype=torch.int64, device="cuda")
    s.render_recursion_photons(camera(desc), w, h, rgb, counts, DEPTH, g, c, buf[guard:guard + need], queue_capacity=100,
                               max_dist=MAX_DIST, nphotons=K, spp=4, jitter=True, children=PATH, environment=True, kinds=7,
                               path_seed=SEED)                                          # raises unless MR_OK
    torch.cuda.synchronize()
    got = counts.tolist()
    assert got[0][:6] == ref.counts[0][:6] and got[0][5] == true_children and got[0][6] == ref.queries[0][0]
    assert got[1][0] == 100 and all(row[0] <= 100 and row[6] <= row[0] for row in got[1:])
    assert bool((buf[:guard] == 0xA5).all()) and bool((buf[guard + need:] == 0xA5).all())
    assert not bool((buf[guard:guard + need] == 0xA5).all())
    fr = frame.FrameRenderer(s, desc, w, h, spp=4, tiled=False, resident_rays=False)
    with pytest.raises(RuntimeError) as e:
        fr.render_specular(depth=DEPTH, lights=lights, environment=ENVS["colour"], path_tracing=True, path_kinds=7, path_seed=SEED,
                           fused="device_photons_path", queue_capacity=100, photon_maps=(g, c), nphotons=K, max_dist=MAX_DIST)
    assert "level 0" in str(e.value) and str(true_children) in str(e.value) and "100" in str(e.value)


@pytest.mark.gpu
@pytest.mark.parametrize("name,children,kinds", [("mirror", SPECULAR, 7), ("flower_drops", PATH, 7)])
def test_replays_from_a_captured_graph(miro, name, children, kinds):
    """After one direct call (it uploads what the scene needs) one mr_render_recursion_photons is captured into a torch.cuda.graph
    on one stream -- a linear graph -- and replayed twice into the same d_rgb and counters, both filled with wrong values before
    each replay: the counters are the direct call's, and on the mirror-only scene at 1 spp so are the bits."""
    import torch
    s, desc, lights = scene(miro, name, "colour")
    g, c = maps_of(miro, name, s, desc)
    spp = 1 if name == "mirror" else 4
    w, h = WINDOWS[spp]
    cap = 4 * w * h * spp
    need = s.recursion_photons_workspace_bytes(camera(desc), w, h, DEPTH, cap, spp=spp, children=children, environment=True)
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    rgb = torch.zeros((w * h, 3), dtype=torch.float32, device="cuda")
    counts = torch.zeros((DEPTH + 1, 8), dtype=torch.int64, device="cuda")

    def launch(stream):
        s.render_recursion_photons(camera(desc), w, h, rgb, counts, DEPTH, g, c, ws, queue_capacity=cap, max_dist=MAX_DIST, nphotons=K,
                                   spp=spp, jitter=spp > 1, children=children, environment=True, kinds=kinds, path_seed=SEED,
                                   stream=stream)

    launch(None)
    torch.cuda.synchronize()
    want_counts, want_rgb = counts.tolist(), rgb.clone()
    assert all(row[0] > 0 for row in want_counts) and want_counts[0][6] > 0 and any(row[6] > 0 for row in want_counts[1:])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        launch(torch.cuda.current_stream())
    for _ in range(2):
        counts.fill_(999999)
        rgb.fill_(-5.0)
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        assert counts.tolist() == want_counts
        if name == "mirror":
            assert np.array_equal(bits(rgb), bits(want_rgb))
        else:
            assert torch.allclose(rgb, want_rgb, rtol=1e-5, atol=1e-6 * float(want_rgb.abs().max()))
