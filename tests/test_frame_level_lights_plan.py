"""render_specular(fused="frame_lights" | "frame_lights_path") without a GPU: what the driver launches, in which order and on which
buffers, recorded by the stand-in scene of tests/test_frame_plan.py (extended by the three launches these routes make), on plain,
table and procedural scenes; what the routes refuse; and that every other value of `fused` launches what it launched before."""
import json
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from miro_amd import binding, frame  # noqa: E402
from test_frame_plan import CASES, DESC, GOLDEN, LIGHTS, SCENES, SQUARE, FakeMap, RecordingScene, run_case, summary  # noqa: E402

W, H, SPP = 16, 8, 2
N = W * H * SPP
INCOHERENT = binding.MR_TRACE_INCOHERENT


class Recorder(RecordingScene):
    """RecordingScene that also does to the counters what mr_render_level_lights and the two level calls would"""

    def launch(self, name, a, kw):
        if name == "render_level_lights":
            n = (kw["y1"] - kw["y0"]) * a[1] * kw["spp"]
        elif name == "trace_level_lights":
            n = a[3]
        elif name == "trace_level_lights_path":
            n = a[4]
        else:
            return super().launch(name, a, kw)
        kw["d_counts"][0] += n
        kw["d_counts"][1] += self.part(n, self.hit)
        if kw["d_out_count"] is not None:
            kw["d_out_count"][0] = self.part(n, self.child)
        return None


def render(scene="plain", tiled=None, bands=None, lens=None, square=False, resident=True, child=(1, 2), **kw):
    sc = Recorder(*SCENES[scene], hit=(3, 4), child=child, image=False)
    fr = frame.FrameRenderer(sc, DESC, W, H, spp=SPP, bands=bands, device=torch.device("cpu"), tiled=tiled, lens=lens,
                             square_lights=SQUARE if square else None, resident_rays=resident)
    for name, t in sorted(vars(fr).items()):                    # the renderer's own buffers go by name
        if isinstance(t, torch.Tensor):
            sc.register(t, name)
    return sc, fr, fr.render_specular(**kw)


def names(sc):
    return [c[0] for c in sc.calls]


def is_buffer(arg, t):
    """a recorded argument is the tensor t"""
    return isinstance(arg, list) and arg[0] == "tensor" and arg[2] == list(t.shape) and arg[3] == str(t.dtype)


@pytest.mark.parametrize("scene", list(SCENES))
@pytest.mark.parametrize("route", ["frame_lights", "frame_lights_path"])
def test_level_0_is_one_frame_launch_then_one_launch_per_level(scene, route):
    """depth 2, half of the rays have a child: set_lights, ONE render_level_lights straight into d_rgb -- no gen_eye_rays, no
    untile_pixels -- then one level launch per further level, adding into d_rgb.  Counts per level come from the launches'
    counters.  A renderer without resident rays serves."""
    path = route == "frame_lights_path"
    kw = dict(path_tracing=True, path_kinds=7, path_seed=5) if path else {}
    sc, fr, per_level = render(scene, resident=False, depth=2, lights=LIGHTS, fused=route, **kw)
    level = "trace_level_lights_path" if path else "trace_level_lights"
    assert names(sc) == ["set_lights", "render_level_lights", level, level]
    assert per_level == [(N, N * 3 // 4), (N // 2, N // 2 * 3 // 4), (N // 4, N // 4 * 3 // 4)]
    (_, a0, k0), (_, a1, k1), (_, a2, k2) = sc.calls[1:]
    # level 0: the whole window, the renderer's sampling, no per-sample output, the children of the route
    assert a0[1:3] == [W, H] and is_buffer(a0[3], fr.d_rgb) and a0[3][1] == "d_rgb"
    assert (k0["y0"], k0["y1"], k0["spp"], k0["jitter"], k0["seed"], k0["tiled"], k0["flags"]) == (0, H, SPP, True, 168, False, 0)
    assert k0["children"] == (binding.MR_LEVEL_PATH if path else binding.MR_LEVEL_SPECULAR) and k0["environment"] is False
    assert k0["d_hits"] is None and k0["d_sample_normal"] is None and k0["d_out_lowres"] is None
    assert (k0["kinds"], k0["path_seed"]) == ((7, 5) if path else (3, 168))
    assert k0["d_out_rays"][2] == [(4 if path else 3) * N, 8] and (k0["d_out_ids"] is not None) == path
    # levels 1 and 2: the children of the level before, into d_rgb, with the incoherent hint; the last one without children
    rgb_at, n_at = (5, 4) if path else (4, 3)
    for a, k, n, last in ((a1, k1, N // 2, False), (a2, k2, N // 4, True)):
        assert a[n_at] == n and a[rgb_at][1] == "d_rgb" and k["flags"] == INCOHERENT and k["spp"] == SPP
        assert k["children"] == (binding.MR_LEVEL_LAST if last else k0["children"]) and (k["d_out_count"] is None) == last
        assert k["d_hits"] is None
    assert a1[0][2] == [N // 2, 8] and a1[1][2] == [N // 2, 3] and a1[2][2] == [N // 2]    # level 1 reads the stored part of the queue
    if path:
        assert a1[3][2] == [N // 2] and (k1["seed"], k1["bounce"], k2["bounce"]) == (5, 1, 2)


def test_tiled_order_needs_no_untile_and_adds_into_d_rgb():
    sc, fr, per_level = render("table", tiled=True, depth=1, lights=LIGHTS, fused="frame_lights")
    assert fr.tiled and names(sc) == ["set_lights", "render_level_lights", "trace_level_lights"]
    assert sc.calls[1][2]["tiled"] is True and sc.calls[1][1][3][1] == "d_rgb" and sc.calls[2][1][4][1] == "d_rgb"
    assert fr.d_slots.data_ptr() != fr.d_rgb.data_ptr()


def test_a_window_depth_0_and_a_queue_that_dies_out():
    sc, fr, per_level = render(bands=[(2, 7)], depth=0, lights=LIGHTS, fused="frame_lights")
    k = sc.calls[1][2]
    assert names(sc) == ["set_lights", "render_level_lights"] and (k["y0"], k["y1"]) == (2, 7)
    assert k["children"] == binding.MR_LEVEL_LAST and k["d_out_count"] is None and k["d_out_rays"] is None
    assert per_level == [(5 * W * SPP, 5 * W * SPP * 3 // 4)]
    sc, fr, per_level = render(child=(0, 1), depth=3, lights=LIGHTS, fused="frame_lights")
    assert names(sc) == ["set_lights", "render_level_lights"] and len(per_level) == 1
    sc, fr, per_level = render(bands=[], depth=3, lights=LIGHTS, fused="frame_lights")
    assert names(sc) == ["set_lights"] and per_level == []


@pytest.mark.parametrize("scene", list(SCENES))
def test_environment_and_photon_maps(scene):
    """environment=dict: the scene's setters, then the frame with environment=True; the path route's queues carry the low-res byte.
    photon_maps in image order: generate() first, the frame writes d_hits (and the bumped normals on a procedural scene), and
    mr_gather_level follows every level on the level's rays, adding into d_rgb."""
    sc, fr, _ = render(scene, depth=1, lights=LIGHTS, fused="frame_lights_path", path_tracing=True, path_kinds=7,
                       environment=dict(bg_color=(0.1, 0.2, 0.3)))
    assert names(sc) == ["set_environment", "get_environment", "set_lights", "render_level_lights", "trace_level_lights_path"]
    k0, k1 = sc.calls[3][2], sc.calls[4][2]
    assert k0["environment"] is True and k1["environment"] is True and k0["d_out_lowres"][2] == [4 * N]
    assert k1["d_lowres"][2] == [N // 2] and k1["d_lowres"][3] == "torch.uint8"
    maps = (FakeMap(), FakeMap())
    sc, fr, per_level = render(scene, depth=1, lights=LIGHTS, fused="frame_lights", photon_maps=maps, nphotons=50, max_dist=2.0)
    assert names(sc) == ["set_lights", "gen_eye_rays", "render_level_lights", "gather_level", "trace_level_lights", "gather_level"]
    k0 = sc.calls[2][2]
    procedural = SCENES[scene][1]
    assert k0["d_hits"][1] == "d_hits" and (k0["d_sample_normal"] is not None) == procedural
    g0, g1 = sc.calls[3], sc.calls[5]
    assert g0[1][2][1] == "d_rays" and g0[1][3][1] == "d_hits" and g0[1][4] == N and g0[1][6][1] == "d_rgb"
    assert (g0[2]["d_normal"] is not None) == procedural and g0[2].get("d_weights") is None and g0[2].get("d_pixels") is None
    assert (g0[2]["nphotons"], g0[2]["max_dist"], g0[2]["spp"]) == (50, 2.0, SPP)
    assert g1[1][4] == N // 2 and g1[1][6][1] == "d_rgb" and g1[2]["d_pixels"] is not None
    assert len(per_level) == 2


def test_refusals_name_the_route_that_serves_the_case():
    ok = dict(depth=1, lights=LIGHTS)
    path = dict(ok, path_tracing=True)
    cases = [
        (dict(lens=dict(aperture=0.1, focus_plane=4.0)), dict(ok, fused="frame_lights"), "batched"),
        (dict(bands=[(0, 2), (4, 6)]), dict(ok, fused="frame_lights"), 'fused="lights"'),
        (dict(bands=[(0, 2), (4, 6)]), dict(path, fused="frame_lights_path"), 'fused="lights_path"'),
        (dict(tiled=True), dict(ok, fused="frame_lights", photon_maps=(FakeMap(), None)), 'fused="lights"'),
        (dict(tiled=True), dict(path, fused="frame_lights_path", photon_maps=(FakeMap(), None)), 'fused="lights_path"'),
        # the checks of "lights" / "lights_path"
        ({}, dict(depth=1, fused="frame_lights"), "lights=[...]"),
        ({}, dict(path, fused="frame_lights"), "path_tracing"),
        ({}, dict(ok, fused="frame_lights_path"), "path_tracing=True"),
        (dict(square=True), dict(ok, fused="frame_lights"), "square lights"),
        ({}, dict(ok, fused="frame_lights", group_octants=True), "group_octants"),
        ({}, dict(ok, fused="frame_lights", surface_children=True), "surface_children=True"),
        ({}, dict(path, fused="frame_lights_path", surface_children=False), "surface_children=False"),
    ]
    for make, kw, word in cases:
        with pytest.raises(ValueError) as e:
            render(**make, **kw)
        assert word in str(e.value), (word, str(e.value))
    # with photon maps in image order and one band range the routes serve
    sc, fr, _ = render(tiled=False, **dict(ok, fused="frame_lights", photon_maps=(FakeMap(), None)))
    assert "render_level_lights" in names(sc)


def test_every_other_value_of_fused_launches_what_it_launched_before():
    """the recorded sequences of tests/golden/render_specular_calls.json hold (tests/test_frame_plan.py checks every case; here one
    of each value of `fused`), no case of them launches the new call -- fused="auto" never picks it -- and the level routes still
    add into d_slots and untile"""
    with open(GOLDEN) as fh:
        golden = json.load(fh)
    for case in CASES:
        assert "render_level_lights" not in golden[case]["calls"], case
    for case in ("plain-nosquare-auto_half_hit", "plain-nosquare-auto_all_hit", "table-nosquare-fused", "procedural-square-path7",
                 "table-nosquare-lights", "plain-nosquare-photon_lights", "procedural-nosquare-depth2"):
        assert summary(run_case(case)) == golden[case], case
    sc, fr, _ = render("table", tiled=True, depth=1, lights=LIGHTS, fused="lights")
    assert names(sc) == ["set_lights", "trace_level_lights", "trace_level_lights", "untile_pixels"]
    assert sc.calls[1][1][4][1] == "d_slots" and sc.calls[2][1][4][1] == "d_slots"
