"""The whole recursive frame through the thin lens on the MI355X (include/miro_hip_lens.h, csrc/mr_frame_lens.hip):
render_specular(fused="frame_lens[_path]" | "device_lens[_path]" | "device_lens_photons[_path]"), mr_render_recursion_lens and
mr_render_recursion_photons_lens.

  "frame_lens[_path]"            against FrameRenderer(lens=...) with fused="lights[_path]", the lens route the parent commit renders:
                                 (rays, shadow rays) per level equal, pixels within the bound the project holds float-atomic sums
                                 to in tests/test_level_lights.py and tests/test_recursion_device.py, rtol 1e-5, atol 1e-6 x max|rgb|
  "device_lens[_path]"           against "frame_lens[_path]": the counters of every level exactly, pixels within that bound, and on
                                 the mirror-only scene at 1 spp -- one addition per pixel and level -- the same bits
  "device_lens_photons[_path]"   against "frame_lens[_path]" with the same maps (the sizes and nphotons of
                                 tests/test_recursion_photons.py): counters and queries per level exactly, pixels within the bound
Depth 0 of mr_render_recursion_lens is mr_render_level_lights_lens with MR_LEVEL_LAST, bit for bit; one capture and two replays of
mr_render_recursion_lens on one stream."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_frame_level_lights import WHOLE  # noqa: E402
from test_frame_lens import APERTURE, focus_of  # noqa: E402
from test_frame_lights import bits, camera  # noqa: E402
from test_level_lights import ENVS, use  # noqa: E402
from test_recursion_device import DEPTH, MIRROR_ONLY, PATH, SEED, SPECULAR, WINDOWS  # noqa: E402
from test_recursion_device import scene as device_scene  # noqa: E402
from test_recursion_photons import K, MAX_DIST, maps_of  # noqa: E402
from test_recursion_photons import scene as photon_scene  # noqa: E402


def lens_of(desc):
    return dict(aperture=APERTURE, focus_plane=focus_of(desc))


def render(s, desc, lights, environment, fused, w, h, spp, depth, children, kinds=7, maps=None, resident=False):
    """One frame of render_specular through the lens.  Returns the renderer with per_level, rgb, and what it saw on the way:
    counts (per level it ran: the level's six counters; on a device route the rows of d_level_counts), pixels (the pixel column
    of every queue of levels >= 1) and queries (per mr_gather_level call: [queries, rays])."""
    import torch
    from miro_amd import frame

    class Spy(frame.FrameRenderer):
        def _level_buffers(self, plan, n, level, last):
            out = super()._level_buffers(plan, n, level, last)
            self.seen_counts.append(out[2])
            return out

        def _level_lights(self, plan, q, level, last, rgb=None):
            if level > 0:
                self.seen_pixels.append(q.pixels)
            return super()._level_lights(plan, q, level, last, rgb=rgb)

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

    s.set_lights(lights)
    s.set_environment(**(environment or {}))
    kw = dict(depth=depth, lights=lights, environment=environment)
    if children == PATH:
        kw.update(path_tracing=True, path_kinds=kinds, path_seed=SEED)
    if maps is not None:
        kw.update(photon_maps=maps, nphotons=K, max_dist=MAX_DIST)
    fr = Spy(s, desc, w, h, spp=spp, tiled=False, lens=lens_of(desc), resident_rays=resident)
    fr.seen_counts, fr.seen_pixels, fr.seen_queries = [], [], []
    if resident:
        fr.generate()
    fr.per_level = fr.render_specular(fused=fused, **kw)
    torch.cuda.synchronize()
    if fused.startswith("device_"):
        fr.counts = fr.d_level_counts[:depth + 1].tolist()
    else:
        fr.counts = [c.tolist() for c in fr.seen_counts]
    fr.pixels = [p.cpu().numpy() for p in fr.seen_pixels]
    fr.queries = [c.tolist() for c in fr.seen_queries]
    fr.rgb = fr.d_rgb.clone()
    return fr


def assert_pixels_close(got, want):
    import torch
    scale = float(want.abs().max())
    assert scale > 0
    assert torch.allclose(got, want, rtol=1e-5, atol=1e-6 * scale), float((got - want).abs().max())


def assert_counts(ref, dev, depth, queries=False):
    """words 0..5 of every level the yardstick ran, word 6 its queries there (without maps 0); the levels it did not run are
    all-zero rows; word 7 is 0; a level's children are the next level's rays"""
    assert len(dev.counts) == depth + 1 and all(len(row) == 8 for row in dev.counts)
    for level, row in enumerate(dev.counts):
        ran = level < len(ref.counts)
        want = (ref.counts[level][:6] + [ref.queries[level][0] if queries else 0]) if ran else [0] * 7
        assert row[:7] == want, (level, row, want)
        assert row[7] == 0
        if level < depth:
            assert dev.counts[level + 1][0] == row[5]
    assert dev.per_level == ref.per_level


# ---- on the MI355X -------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("route", ["lights", "lights_path"])
@pytest.mark.parametrize("name,env,depth", WHOLE)
def test_whole_frames(miro, name, env, depth, route):
    """48 x 32 at 1 and 2 spp: "frame_lens[_path]" against the batched lens route "lights[_path]" of a renderer with the same lens,
    then "device_lens[_path]" against "frame_lens[_path]"."""
    children = PATH if route == "lights_path" else SPECULAR
    lens_route = "lens_path" if children == PATH else "lens"
    for spp in (1, 2):
        s, desc, lights = use(miro, name, env)
        args = (s, desc, lights, ENVS[env])
        old = render(*args, route, 48, 32, spp, depth, children, resident=True)
        fr = render(*args, "frame_" + lens_route, 48, 32, spp, depth, children)
        dev = render(*args, "device_" + lens_route, 48, 32, spp, depth, children)
        print("per_level", old.per_level, "max", float(old.rgb.max()))
        assert len(old.per_level) >= 2 and all(n > 0 and sh > 0 for n, sh in old.per_level) and old.per_level[0][0] == 48 * 32 * spp
        assert fr.per_level == old.per_level
        assert_pixels_close(fr.rgb, old.rgb)
        assert_counts(fr, dev, depth)
        assert_pixels_close(dev.rgb, fr.rgb)
    use(miro, name, None)


@pytest.mark.gpu
@pytest.mark.parametrize("children", [SPECULAR, PATH], ids=["specular", "path"])
def test_mirror_only_at_one_sample_is_the_yardsticks_bits(miro, children):
    """The mirror-only scene of tests/test_recursion_device.py at 1 spp: one ray per pixel and level (asserted from the yardstick's
    own queues), so a pixel receives one addition per level and d_rgb is compared on its bits."""
    s, desc, lights = device_scene(miro, "mirror", "colour")
    w, h = WINDOWS[1]
    route = "lens_path" if children == PATH else "lens"
    args = (s, desc, lights, ENVS["colour"])
    fr = render(*args, "frame_" + route, w, h, 1, DEPTH, children, kinds=MIRROR_ONLY)
    dev = render(*args, "device_" + route, w, h, 1, DEPTH, children, kinds=MIRROR_ONLY)
    assert len(fr.pixels) == DEPTH and len(fr.pixels[0]) > 256 and all(len(p) > 0 for p in fr.pixels)
    for level, p in enumerate(fr.pixels, 1):
        assert len(np.unique(p)) == len(p), level
    assert_counts(fr, dev, DEPTH)
    assert np.array_equal(bits(dev.rgb), bits(fr.rgb)) and float(fr.rgb.abs().max()) > 0


@pytest.mark.gpu
@pytest.mark.parametrize("name,env", [("flower_drops", "image"), ("mirror", "colour")])
def test_depth_0_is_the_level_0_lens_frame_bit_for_bit(miro, name, env):
    """mr_render_recursion_lens at depth 0 against mr_render_level_lights_lens with MR_LEVEL_LAST: pixels and the five counters;
    no workspace"""
    import torch
    s, desc, lights = device_scene(miro, name, env)
    w, h = WINDOWS[4]
    lens = lens_of(desc)
    rgb = torch.full((w * h, 3), 7.0, dtype=torch.float32, device="cuda")
    want = torch.full((w * h, 3), 9.0, dtype=torch.float32, device="cuda")
    counts = torch.full((1, 8), 999, dtype=torch.int64, device="cuda")
    five = torch.zeros(5, dtype=torch.int64, device="cuda")
    s.render_recursion_lens(camera(desc), w, h, rgb, counts, 0, lens["aperture"], lens["focus_plane"], spp=4, jitter=True,
                            environment=True, children=0)
    s.render_level_lights_lens(camera(desc), w, h, want, lens["aperture"], lens["focus_plane"], spp=4, jitter=True, environment=True,
                               d_counts=five)
    torch.cuda.synchronize()
    assert np.array_equal(bits(rgb), bits(want)) and float(want.abs().max()) > 0
    got = counts[0].tolist()
    assert got[:5] == five.tolist() and got[5:] == [0, 0, 0] and got[0] == w * h * 4 and got[1] > 0


@pytest.mark.gpu
@pytest.mark.parametrize("children", [SPECULAR, PATH], ids=["specular", "path"])
@pytest.mark.parametrize("name", ["glass", "stone"])
def test_with_photon_maps(miro, name, children):
    """"device_lens_photons[_path]" against "frame_lens[_path]" with the same maps, 40 x 24 x 2, depth 3: the glass room of
    tests/test_recursion_photons.py, and the stone room, where level 0's queries read the bumped-normal buffer"""
    s, desc, lights = photon_scene(miro, name, None)
    maps = maps_of(miro, name, s, desc)
    route = "lens_path" if children == PATH else "lens"
    args = (s, desc, lights, None)
    fr = render(*args, "frame_" + route, 40, 24, 2, DEPTH, children, maps=maps, resident=True)
    dev = render(*args, "device_lens_photons" + route[4:], 40, 24, 2, DEPTH, children, maps=maps)
    print("per_level", fr.per_level, "queries", fr.queries)
    assert len(fr.queries) == len(fr.counts) and all(q[1] == c[0] for q, c in zip(fr.queries, fr.counts))
    assert fr.queries[0][0] > 0 and any(q[0] > 0 for q in fr.queries[1:]), fr.queries
    assert_counts(fr, dev, DEPTH, queries=True)
    assert_pixels_close(dev.rgb, fr.rgb)
    plain = render(*args, "device_" + route, 40, 24, 2, DEPTH, children)             # the term is there
    assert float((dev.rgb - plain.rgb).abs().max()) > 1e-3 * float(fr.rgb.abs().max())


@pytest.mark.gpu
def test_replays_from_a_captured_graph(miro):
    """After one direct call one mr_render_recursion_lens on the mirror scene at 1 spp is captured into a torch.cuda.graph on one
    stream and replayed twice into the same d_rgb and counters, both filled with wrong values before each replay: counters and
    bits are the direct call's."""
    import torch
    s, desc, lights = device_scene(miro, "mirror", "colour")
    w, h = WINDOWS[1]
    lens = lens_of(desc)
    cap = 3 * w * h
    ws = torch.empty(s.recursion_workspace_bytes(DEPTH, cap, children=SPECULAR, environment=True), dtype=torch.uint8, device="cuda")
    rgb = torch.zeros((w * h, 3), dtype=torch.float32, device="cuda")
    counts = torch.zeros((DEPTH + 1, 8), dtype=torch.int64, device="cuda")

    def launch(stream):
        s.render_recursion_lens(camera(desc), w, h, rgb, counts, DEPTH, lens["aperture"], lens["focus_plane"], d_workspace=ws,
                                queue_capacity=cap, spp=1, children=SPECULAR, environment=True, stream=stream)

    launch(None)
    torch.cuda.synchronize()
    want_counts, want_rgb = counts.tolist(), rgb.clone()
    assert all(row[0] > 0 for row in want_counts) and float(want_rgb.abs().max()) > 0
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        launch(torch.cuda.current_stream())
    for _ in range(2):
        counts.fill_(999999)
        rgb.fill_(-5.0)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        assert counts.tolist() == want_counts
        assert torch.allclose(rgb, want_rgb, rtol=1e-5, atol=1e-6 * float(want_rgb.abs().max()))
