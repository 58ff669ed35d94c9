"""mr_render_recursion_passes / mr_render_recursion_photons_passes on the MI355X (include/miro_hip_passes.h,
csrc/mr_frame_passes.hip): a frame of S samples per pixel in passes, whose samples have one numbering that no cut into passes or
calls changes.

Windows 24 x 16 and 40 x 24, depth 3 (and depth 0 where the result is bits), the scenes and helpers of
tests/test_recursion_device.py, test_recursion_lens.py and test_recursion_photons.py (imported, not copied).

  counts      words 0..5 (with maps 0..6) of every level, summed over the passes, EXACTLY those of the yardstick
  pixels      bit for bit where the float operations are the same sequence (depth 0: one pass = the parent call; two equal
              passes of a power-of-two S, because (a + b) / 4 = a / 4 + b / 4 exactly; a frame continued by a second call);
              elsewhere rtol = 1e-5, atol = 1e-6 x max|rgb|, the bound the project holds reordered float pixel sums to
  yardsticks  S a power of two: the existing one-call frame at spp = S.  S = 7, 11: the per-level route generate() +
              render_specular(fused="lights" | "lights_path") at spp = S, which makes the same sample keys and ray ids"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_frame_lights import bits, camera  # noqa: E402
from test_level_lights import ENVS  # noqa: E402
from test_recursion_device import DEPTH, PATH, SEED, SPECULAR, WINDOWS  # noqa: E402
from test_recursion_device import scene as device_scene  # noqa: E402
from test_recursion_lens import lens_of  # noqa: E402
from test_recursion_photons import K, MAX_DIST, maps_of  # noqa: E402
from test_recursion_photons import scene as photon_scene  # noqa: E402


FAN = 4 ** DEPTH                                        # rays per sample that no queue of a path-traced frame can exceed


def setup(miro, name, env, photons=False):
    """(scene, description, lights, maps or None) with the lights and the environment set"""
    s, desc, lights = (photon_scene if photons else device_scene)(miro, name, env)
    return s, desc, lights, maps_of(miro, name, s, desc) if photons else None


def sampling(children, env, capacity):
    return dict(jitter=True, children=children, environment=env is not None, kinds=7, path_seed=SEED, queue_capacity=capacity)


def workspace(s, desc, w, h, spp, depth, children, env, capacity, maps):
    import torch
    if maps is not None:
        need = s.recursion_photons_workspace_bytes(camera(desc), w, h, depth, capacity, spp=spp, children=children,
                                                   environment=env is not None)
    else:
        need = s.recursion_workspace_bytes(depth, capacity, children=children, environment=env is not None)
    return torch.empty(max(need, 16), dtype=torch.uint8, device="cuda")


def parent(s, desc, w, h, spp, depth, children, env, lens=None, maps=None):
    """the existing one-call frame: (rgb, counts [depth + 1][8])"""
    import torch
    cap = FAN * w * h * spp
    rgb = torch.full((w * h, 3), 7.0, dtype=torch.float32, device="cuda")
    counts = torch.full((depth + 1, 8), 999, dtype=torch.int64, device="cuda")
    ws = workspace(s, desc, w, h, spp, depth, children, env, cap, maps)
    kw = dict(sampling(children, env, cap), spp=spp)
    if depth == 0:
        kw["children"] = 0
    cam = camera(desc)
    if maps is not None and lens is not None:
        s.render_recursion_photons_lens(cam, w, h, rgb, counts, depth, maps[0], maps[1], ws, lens["aperture"], lens["focus_plane"],
                                        max_dist=MAX_DIST, nphotons=K, **kw)
    elif maps is not None:
        s.render_recursion_photons(cam, w, h, rgb, counts, depth, maps[0], maps[1], ws, max_dist=MAX_DIST, nphotons=K, **kw)
    elif lens is not None:
        s.render_recursion_lens(cam, w, h, rgb, counts, depth, lens["aperture"], lens["focus_plane"], d_workspace=ws if depth else None, **kw)
    else:
        s.render_recursion(cam, w, h, rgb, counts, depth, d_workspace=ws if depth else None, **kw)
    torch.cuda.synchronize()
    return rgb, counts.tolist()


def passes(miro, s, desc, w, h, S, spp, depth, children, env, lens=None, maps=None, begin=0, end=None, rgb=None, capacity=None,
           stream=None, ws=None, counts=None):
    """the call under test: (rgb, counts [passes][depth + 1][8], plan)"""
    import torch
    from miro_amd import binding
    plan = binding.passes_plan(spp, S, begin, end)
    cap = FAN * w * h * spp if capacity is None else capacity
    if rgb is None:
        rgb = torch.full((w * h, 3), 7.0, dtype=torch.float32, device="cuda")
    if counts is None:
        counts = torch.full((len(plan), depth + 1, 8), 999, dtype=torch.int64, device="cuda")
    if ws is None:
        ws = workspace(s, desc, w, h, spp, depth, children, env, cap, maps)
    kw = dict(sampling(children, env, cap), spp=spp, sample_begin=begin, sample_end=end, lens=lens, stream=stream)
    if depth == 0:
        kw["children"] = 0
    if maps is not None:
        s.render_recursion_photons_passes(camera(desc), w, h, rgb, counts, depth, S, maps[0], maps[1], ws, max_dist=MAX_DIST, nphotons=K, **kw)
    else:
        s.render_recursion_passes(camera(desc), w, h, rgb, counts, depth, S, d_workspace=ws if depth else None, **kw)
    if stream is None:
        torch.cuda.synchronize()
        return rgb, counts.tolist(), plan
    return rgb, counts, plan


def summed(blocks, words=6):
    """per level, words [0, words) summed over the passes"""
    return [[sum(b[level][k] for b in blocks) for k in range(words)] for level in range(len(blocks[0]))]


def close(got, want):
    import torch
    scale = float(want.abs().max())
    assert scale > 0
    return bool(torch.allclose(got, want, rtol=1e-5, atol=1e-6 * scale))


def assert_close(got, want):
    assert close(got, want), float((got - want).abs().max())


def same(got, want):
    return np.array_equal(bits(got), bits(want))


# ---- one pass is the parent call -----------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("depth", [0, DEPTH])
@pytest.mark.parametrize("kind", ["plain", "lens", "photons"])
@pytest.mark.parametrize("spp", [1, 4])
def test_one_pass_is_the_parent_call(miro, spp, kind, depth):
    """S = spp, range [0, S): d_rgb and the counts are mr_render_recursion's, _lens' and _photons' -- at depth 0 on their bits, at
    depth 3 the counts exactly and the pixels within the bound (levels >= 1 add with float atomics in both)"""
    children = PATH if spp == 4 else SPECULAR
    s, desc, lights, maps = setup(miro, "glass", "colour", photons=kind == "photons")
    w, h = WINDOWS[spp]
    lens = lens_of(desc) if kind == "lens" else None
    want_rgb, want_counts = parent(s, desc, w, h, spp, depth, children, "colour", lens, maps)
    rgb, counts, plan = passes(miro, s, desc, w, h, spp, spp, depth, children, "colour", lens, maps)
    print("counts", want_counts)
    assert plan == [(0, spp)] and len(counts) == 1
    assert counts[0] == want_counts and want_counts[0][0] == w * h * spp and want_counts[0][1] > 0
    assert depth == 0 or all(row[0] > 0 for row in want_counts)
    assert kind != "photons" or want_counts[0][6] > 0
    if depth == 0:
        assert same(rgb, want_rgb) and float(want_rgb.abs().max()) > 0
    else:
        assert_close(rgb, want_rgb)


# ---- split equals whole, S a power of two ----------------------------------------------------------------------------------------
SPLIT = [("glass", SPECULAR, False, None), ("glass", PATH, True, "colour"), ("mirror", SPECULAR, True, None),
         ("flower_drops", PATH, False, "image")]


@pytest.mark.gpu
@pytest.mark.parametrize("depth", [0, DEPTH])
@pytest.mark.parametrize("name,children,with_lens,env", SPLIT, ids=["glass-specular", "glass-path-lens-colour", "mirror-specular-lens",
                                                                     "flower-path-image"])
def test_split_equals_whole_at_4_samples(miro, name, children, with_lens, env, depth):
    """S = 4 as 4 x 1 and as 2 x 2 against the existing call at spp = 4 with the same seeds.  The precondition, with existing calls
    only: the frame that repeats sample 0 four times -- spp = 1, whose mean of four equal terms is the term -- differs from the
    yardstick by more than the bound, so a wrong numbering (every pass drawing sample 0's numbers) would be seen."""
    s, desc, lights, _ = setup(miro, name, env)
    w, h = WINDOWS[4]
    lens = lens_of(desc) if with_lens else None
    want_rgb, want_counts = parent(s, desc, w, h, 4, depth, children, env, lens)
    repeat_rgb, _ = parent(s, desc, w, h, 1, depth, children, env, lens)
    assert not close(repeat_rgb, want_rgb)
    print("counts", want_counts)
    assert depth == 0 or all(row[0] > 0 for row in want_counts)
    for spp in (1, 2):
        rgb, counts, plan = passes(miro, s, desc, w, h, 4, spp, depth, children, env, lens)
        assert plan == [(b, spp) for b in range(0, 4, spp)]
        assert summed(counts) == [row[:6] for row in want_counts], spp
        assert all(b[level + 1][0] == b[level][5] for b in counts for level in range(depth))     # per pass, children are the next rays
        if depth == 0 and spp == 2:
            assert same(rgb, want_rgb)
        else:
            assert_close(rgb, want_rgb)


# ---- split equals whole, other S ---------------------------------------------------------------------------------------------------
def yardstick(miro, s, desc, lights, env, w, h, S, children, lens=None, maps=None):
    """generate() + render_specular(fused="lights" | "lights_path") at spp = S: (rgb, counts per level [0..6): the level's six
    counters, queries per level or None)"""
    import torch
    from miro_amd import frame

    class Spy(frame.FrameRenderer):
        def _level_buffers(self, plan, n, level, last):
            out = super()._level_buffers(plan, n, level, last)
            self.seen_counts.append(out[2])
            return out

        def _gather(self, plan, q, hits, normal, rgb):
            real, spy = self.scene.gather_level, self

            def counted(*a, **kw):
                cnt = torch.zeros(2, dtype=torch.int64, device=spy.device)
                spy.seen_queries.append(cnt)
                return real(*a, d_counts=cnt, **kw)
            if plan.photon_maps is None:
                return super()._gather(plan, q, hits, normal, rgb)
            self.scene.gather_level = counted
            try:
                super()._gather(plan, q, hits, normal, rgb)
            finally:
                del self.scene.gather_level

    kw = dict(depth=DEPTH, lights=lights, environment=ENVS[env])
    if children == PATH:
        kw.update(path_tracing=True, path_kinds=7, path_seed=SEED)
    if maps is not None:
        kw.update(photon_maps=maps, nphotons=K, max_dist=MAX_DIST)
    fr = Spy(s, desc, w, h, spp=S, tiled=False, lens=lens)
    fr.seen_counts, fr.seen_queries = [], []
    fr.generate()
    fr.per_level = fr.render_specular(fused="lights_path" if children == PATH else "lights", **kw)
    torch.cuda.synchronize()
    return fr, [c.tolist()[:6] for c in fr.seen_counts], [c.tolist()[0] for c in fr.seen_queries] if maps is not None else None


OTHER = [(7, "glass", SPECULAR, False, None, False), (11, "glass", PATH, True, "colour", False), (7, "glass", SPECULAR, False, None, True),
         (11, "flower_drops", PATH, False, "image", False)]


@pytest.mark.gpu
@pytest.mark.parametrize("S,name,children,with_lens,env,photons", OTHER, ids=["7-glass-specular", "11-glass-path-lens-colour",
                                                                               "7-glassroom-photons", "11-flower-path-image"])
def test_split_equals_whole_at_7_and_11_samples(miro, S, name, children, with_lens, env, photons):
    """S = 7 (passes 4, 2, 1) and S = 11 (4, 4, 2, 1) through render_specular(fused="device_*", samples=S) of a renderer at spp = 4,
    against the per-level route at spp = S: counts summed over the passes exactly, per_level, pixels within the bound"""
    from miro_amd import frame
    s, desc, lights, maps = setup(miro, name, env, photons=photons)
    w, h = WINDOWS[4]
    lens = lens_of(desc) if with_lens else None
    ref, want_counts, want_queries = yardstick(miro, s, desc, lights, env, w, h, S, children, lens, maps)
    print("per_level", ref.per_level, "counts", want_counts, "queries", want_queries)
    assert len(ref.per_level) == DEPTH + 1 and ref.per_level[0][0] == w * h * S
    route = "device_" + ("lens" if with_lens else "photons" if photons else "lights") + ("_path" if children == PATH else "")
    kw = dict(depth=DEPTH, lights=lights, environment=ENVS[env], samples=S)
    if children == PATH:
        kw.update(path_tracing=True, path_kinds=7, path_seed=SEED)
    if maps is not None:
        kw.update(photon_maps=maps, nphotons=K, max_dist=MAX_DIST)
    fr = frame.FrameRenderer(s, desc, w, h, spp=4, jitter=True, tiled=False, lens=lens, resident_rays=False)
    per_level = fr.render_specular(fused=route, **kw)
    n_passes = 3 if S == 7 else 4
    blocks = fr.d_pass_counts[:n_passes].tolist()
    assert [b[0][0] // (w * h) for b in blocks] == ([4, 2, 1] if S == 7 else [4, 4, 2, 1])
    assert summed(blocks) == want_counts
    assert per_level == ref.per_level
    if photons:
        got_queries = [row[0] for row in summed([[[r[6]] for r in b] for b in blocks], 1)]
        assert got_queries == want_queries and want_queries[0] > 0 and any(q > 0 for q in want_queries[1:])
    assert_close(fr.d_rgb, ref.d_rgb)


# ---- continuing a frame ------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("depth", [0, DEPTH])
@pytest.mark.parametrize("with_lens", [False, True], ids=["pinhole", "lens"])
def test_a_second_call_continues_the_frame(miro, with_lens, depth):
    """[0, 4) and then [4, 8) of S = 8 against one call [0, 8): at depth 0 the same stores and adds, bit for bit; at depth 3 within
    the bound.  The first call alone is not the frame (the second one adds)."""
    s, desc, lights, _ = setup(miro, "glass", "colour")
    w, h = WINDOWS[4]
    lens = lens_of(desc) if with_lens else None
    whole, whole_counts, plan = passes(miro, s, desc, w, h, 8, 4, depth, PATH, "colour", lens)
    assert plan == [(0, 4), (4, 4)]
    rgb, first, _ = passes(miro, s, desc, w, h, 8, 4, depth, PATH, "colour", lens, begin=0, end=4)
    half = rgb.clone()
    rgb, second, plan = passes(miro, s, desc, w, h, 8, 4, depth, PATH, "colour", lens, begin=4, end=8, rgb=rgb)
    assert plan == [(4, 4)] and first + second == whole_counts
    assert not close(half, whole)
    if depth == 0:
        assert same(rgb, whole)
    else:
        assert_close(rgb, whole)


# ---- graph capture -----------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("depth", [0, DEPTH])
def test_replays_from_a_captured_graph(miro, depth):
    """S = 7 in passes of 4, 2, 1 through the lens with path-traced children: one direct call (it uploads what the scene needs),
    then the call captured on one stream and replayed twice into d_rgb and counters filled with wrong values before each replay"""
    import torch
    s, desc, lights, _ = setup(miro, "glass", "colour")
    w, h = WINDOWS[4]
    lens = lens_of(desc)
    cap = FAN * w * h * 4
    ws = workspace(s, desc, w, h, 4, depth, PATH, "colour", cap, None)
    rgb = torch.zeros((w * h, 3), dtype=torch.float32, device="cuda")
    counts = torch.zeros((3, depth + 1, 8), dtype=torch.int64, device="cuda")
    args = (miro, s, desc, w, h, 7, 4, depth, PATH, "colour", lens)
    passes(*args, rgb=rgb, ws=ws, counts=counts, capacity=cap)
    want_rgb, want_counts = rgb.clone(), counts.tolist()
    assert [b[0][0] for b in want_counts] == [w * h * 4, w * h * 2, w * h] and float(want_rgb.abs().max()) > 0
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        passes(*args, rgb=rgb, ws=ws, counts=counts, capacity=cap, stream=torch.cuda.current_stream())
    for _ in range(2):
        counts.fill_(999999)
        rgb.fill_(-5.0)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        assert counts.tolist() == want_counts
        if depth == 0:
            assert same(rgb, want_rgb)
        else:
            assert_close(rgb, want_rgb)


# ---- truncation --------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_a_capacity_of_100_shows_in_each_pass_own_counters(miro):
    """S = 6 in passes of 4 and 2 on the glass sphere: with queue_capacity = 100 each pass's [0][5] is that pass's true number of
    children (the un-truncated run's), its level 1 runs exactly 100 rays, no level holds more, and the guard regions around the
    declared workspace keep their pattern.  render_specular(samples=6) raises RuntimeError naming the pass.  Once: a bounds check."""
    import torch
    from miro_amd import frame
    s, desc, lights, _ = setup(miro, "glass", "colour")
    w, h = WINDOWS[4]
    _, true_counts, plan = passes(miro, s, desc, w, h, 6, 4, DEPTH, PATH, "colour")
    assert plan == [(0, 4), (4, 2)] and all(b[0][5] > 100 for b in true_counts)
    need = s.recursion_workspace_bytes(DEPTH, 100, children=PATH, environment=True)
    guard = 4096
    buf = torch.full((guard + need + guard,), 0xA5, dtype=torch.uint8, device="cuda")
    _, got, _ = passes(miro, s, desc, w, h, 6, 4, DEPTH, PATH, "colour", capacity=100, ws=buf[guard:guard + need])
    for b, t in zip(got, true_counts):
        assert b[0] == t[0] and b[1][0] == 100 and all(row[0] <= 100 for row in b[1:])
    assert bool((buf[:guard] == 0xA5).all()) and bool((buf[guard + need:] == 0xA5).all())
    fr = frame.FrameRenderer(s, desc, w, h, spp=4, tiled=False, resident_rays=False)
    with pytest.raises(RuntimeError) as e:
        fr.render_specular(depth=DEPTH, lights=lights, environment=ENVS["colour"], path_tracing=True, path_kinds=7, path_seed=SEED,
                           fused="device_lights_path", queue_capacity=100, samples=6)
    assert "pass 0" in str(e.value) and "level 0" in str(e.value) and str(true_counts[0][0][5]) in str(e.value) and "100" in str(e.value)
