"""FrameRenderer.render_specular(fused="lights"): the launch sequence of the route whose every level is one
mr_trace_level_lights, on torch's CPU device with the recording stand-in of tests/test_frame_plan.py -- which buffer goes where,
what follows the launch with photon maps, and what the route refuses.  (The existing routes' records are pinned by
tests/golden/render_specular_calls.json and are not touched here.)"""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_frame_plan import DESC, LIGHTS, SCENES, SPP, SQUARE, FakeMap, H, RecordingScene, W  # noqa: E402

from miro_amd import binding, frame  # noqa: E402


class LevelLightsScene(RecordingScene):
    """RecordingScene that also moves trace_level_lights' counters: [0] += rays, [1] += hits x lights; d_out_count = children"""

    n_lights = len(LIGHTS)

    def launch(self, name, a, kw):
        if name == "trace_level_lights":
            n = a[3]
            self.__dict__.setdefault("raw", []).append((a, kw))         # the tensors themselves: the record keeps labels only
            kw["d_counts"][0] += n
            kw["d_counts"][1] += self.part(n, self.hit) * self.n_lights
            if kw["d_out_count"] is not None:
                kw["d_out_count"][0] = self.part(n, self.child)
            return None
        return super().launch(name, a, kw)


def run(scene, square=False, **kw):
    sc = LevelLightsScene(*SCENES[scene], hit=(3, 4), child=(1, 2), image=False)
    fr = frame.FrameRenderer(sc, DESC, W, H, spp=SPP, device=torch.device("cpu"), square_lights=SQUARE if square else None)
    for name, t in sorted(vars(fr).items()):
        if isinstance(t, torch.Tensor):
            sc.register(t, name)
    return sc, fr, fr.render_specular(**kw)


def label(sc, encoded):
    """the label RecordingScene gave a tensor argument"""
    return None if encoded is None else encoded[1]


@pytest.mark.parametrize("scene", list(SCENES))
def test_every_level_is_one_launch_on_every_scene(scene):
    """depth 2 on the plain, table and procedural scenes: set_lights, then three trace_level_lights; the last one has
    children = MR_LEVEL_LAST and no output queue; each level's queue is the previous level's output buffers; every level adds to
    the renderer's d_rgb; per_level is (rays, shadow rays)"""
    sc, fr, per_level = run(scene, depth=2, lights=LIGHTS, fused="lights")
    assert [c[0] for c in sc.calls] == ["set_lights"] + ["trace_level_lights"] * 3
    levels = sc.calls[1:]
    n = W * H * SPP
    want = []
    for k, (_, a, kw) in enumerate(levels):
        assert a[3] == n and label(sc, a[4]) == "d_rgb" and kw["spp"] == SPP and kw["environment"] is False
        assert kw["children"] == (binding.MR_LEVEL_LAST if k == 2 else binding.MR_LEVEL_SPECULAR)
        assert kw["d_hits"] is None and kw["d_normal"] is None
        assert kw["flags"] == (binding.MR_TRACE_INCOHERENT if k else 0)
        want.append([n, (n * 3 // 4) * len(LIGHTS)])
        n = n // 2
    assert per_level == [tuple(w) for w in want]
    assert label(sc, levels[0][1][0]) == "d_rays" and levels[0][1][1] is None and levels[0][1][2] is None
    for (pa, pkw), (na, _) in zip(sc.raw, sc.raw[1:]):
        out = [pkw[k] for k in ("d_out_rays", "d_out_weights", "d_out_pixels")]
        assert [t.data_ptr() for t in na[:3]] == [o.data_ptr() for o in out]                # the same storage ...
        assert [t.shape[0] for t in na[:3]] == [na[3]] * 3 and [o.shape[0] for o in out] == [3 * pa[3]] * 3     # ... its leading rows
    last = levels[2][2]
    assert last["d_out_rays"] is None and last["d_out_weights"] is None and last["d_out_pixels"] is None and last["d_out_count"] is None


def test_environment_in_every_form():
    sc, _, _ = run("table", depth=2, lights=LIGHTS, fused="lights", environment=dict(bg_color=(0.1, 0.2, 0.3)))
    assert [c[0] for c in sc.calls] == ["set_environment", "get_environment", "set_lights"] + ["trace_level_lights"] * 3
    assert all(c[2]["environment"] is True for c in sc.calls[3:])
    sc, _, _ = run("plain", depth=1, lights=LIGHTS, fused="lights", environment=True)
    assert [c[0] for c in sc.calls] == ["get_environment", "set_lights"] + ["trace_level_lights"] * 2
    assert all(c[2]["environment"] is True for c in sc.calls[2:])


@pytest.mark.parametrize("scene", ["table", "procedural"])
def test_photon_maps_follow_each_level(scene):
    """each level is followed by gather_level on the hit records the level wrote (level 0: the renderer's d_hits), with the
    level's queue, and with the level's normal buffer on a procedural scene only"""
    sc, _, per_level = run(scene, depth=2, lights=LIGHTS, fused="lights", photon_maps=(FakeMap(), None), nphotons=50, max_dist=2.0)
    assert [c[0] for c in sc.calls] == ["set_lights"] + ["trace_level_lights", "gather_level"] * 3
    assert len(per_level) == 3
    for k in range(3):
        (_, la, lkw), (_, ga, gkw) = sc.calls[1 + 2 * k], sc.calls[2 + 2 * k]
        assert lkw["d_hits"] is not None and ga[3] == lkw["d_hits"] and ga[2] == la[0] and ga[4] == la[3]
        assert (label(sc, lkw["d_hits"]) == "d_hits") == (k == 0)
        assert gkw["d_weights"] == la[1] and gkw["d_pixels"] == la[2] and gkw["nphotons"] == 50 and gkw["max_dist"] == 2.0
        if scene == "procedural":
            assert lkw["d_normal"] is not None and gkw["d_normal"] == lkw["d_normal"]
        else:
            assert lkw["d_normal"] is None and gkw["d_normal"] is None


@pytest.mark.parametrize("kw,square,word", [
    (dict(path_tracing=True), False, "path_tracing"), (dict(group_octants=True), False, "group_octants"),
    (dict(surface_children=True), False, "surface_children"), (dict(), True, "square lights")])
def test_what_the_route_refuses(kw, square, word):
    with pytest.raises(ValueError) as e:
        run("plain", square=square, depth=2, lights=LIGHTS, fused="lights", **kw)
    assert word in str(e.value) and "fused=\"lights\"" in str(e.value)


def test_it_needs_a_light_list():
    with pytest.raises(ValueError) as e:
        run("plain", depth=2, fused="lights")
    assert "lights=[...]" in str(e.value)


def test_the_other_routes_never_take_it():
    """fused=True / "auto" / False launch what they launched before: no trace_level_lights"""
    for fused in (False, True, "auto"):
        sc, _, _ = run("plain", depth=2, fused=fused)
        assert "trace_level_lights" not in [c[0] for c in sc.calls]
