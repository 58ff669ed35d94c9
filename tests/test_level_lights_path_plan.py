"""FrameRenderer.render_specular(fused="lights_path"): the launch sequence of the route whose every level is one
mr_trace_level_lights_path, on torch's CPU device with the recording stand-in of tests/test_frame_plan.py -- which buffer goes where
(the path tracer's ids and the low-res byte included), what follows the launch with photon maps, and what the route refuses.  (The
existing routes' records are pinned by tests/golden/render_specular_calls.json and tests/test_level_lights_plan.py and are not
touched here.)"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_frame_plan import DESC, LIGHTS, SCENES, SPP, SQUARE, FakeMap, H, RecordingScene, W  # noqa: E402

from miro_amd import binding, frame  # noqa: E402

NAME = "trace_level_lights_path"


class LevelPathScene(RecordingScene):
    """RecordingScene that also moves trace_level_lights_path's counters: [0] += rays, [1] += hits x lights; d_out_count = children"""

    n_lights = len(LIGHTS)

    def launch(self, name, a, kw):
        if name == NAME:
            n = a[4]
            self.__dict__.setdefault("raw", []).append((a, kw))         # the tensors themselves: the record keeps labels only
            kw["d_counts"][0] += n
            kw["d_counts"][1] += self.part(n, self.hit) * self.n_lights
            if kw["d_out_count"] is not None:
                kw["d_out_count"][0] = self.part(n, self.child)
            return None
        return super().launch(name, a, kw)


def run(scene, square=False, image=False, **kw):
    sc = LevelPathScene(*SCENES[scene], hit=(3, 4), child=(1, 2), image=image)
    fr = frame.FrameRenderer(sc, DESC, W, H, spp=SPP, device=torch.device("cpu"), square_lights=SQUARE if square else None)
    for name, t in sorted(vars(fr).items()):
        if isinstance(t, torch.Tensor):
            sc.register(t, name)
    return sc, fr, fr.render_specular(**kw)


def label(sc, encoded):
    """the label RecordingScene gave a tensor argument"""
    return None if encoded is None else encoded[1]


PATH = dict(lights=LIGHTS, fused="lights_path", path_tracing=True)


@pytest.mark.parametrize("scene", list(SCENES))
def test_every_level_is_one_launch_on_every_scene(scene):
    """depth 2 on the plain, table and procedural scenes: set_lights, then three trace_level_lights_path; the last one has
    children = MR_LEVEL_LAST and no output queue; each level's queue -- rays, weights, pixels and ids -- is the previous level's
    output buffers, four slots per ray; seed, kinds and the level as bounce go with every launch; every level adds to the
    renderer's d_rgb; without an environment no low-res byte exists; per_level is (rays, shadow rays)"""
    sc, fr, per_level = run(scene, depth=2, path_seed=5, path_kinds=5, **PATH)
    assert [c[0] for c in sc.calls] == ["set_lights"] + [NAME] * 3
    levels = sc.calls[1:]
    n = W * H * SPP
    want = []
    for k, (_, a, kw) in enumerate(levels):
        assert a[4] == n and label(sc, a[5]) == "d_rgb" and kw["spp"] == SPP and kw["environment"] is False
        assert kw["children"] == (binding.MR_LEVEL_LAST if k == 2 else binding.MR_LEVEL_PATH)
        assert kw["seed"] == 5 and kw["kinds"] == 5 and kw["bounce"] == k
        assert kw["d_hits"] is None and kw["d_normal"] is None and kw["d_lowres"] is None and kw["d_out_lowres"] is None
        assert kw["flags"] == (binding.MR_TRACE_INCOHERENT if k else 0)
        want.append([n, (n * 3 // 4) * len(LIGHTS)])
        n = n // 2
    assert per_level == [tuple(w) for w in want]
    assert label(sc, levels[0][1][0]) == "d_rays" and levels[0][1][1:4] == [None, None, None]
    for (pa, pkw), (na, _) in zip(sc.raw, sc.raw[1:]):
        out = [pkw[k] for k in ("d_out_rays", "d_out_weights", "d_out_pixels", "d_out_ids")]
        assert [t.data_ptr() for t in na[:4]] == [o.data_ptr() for o in out]                # the same storage ...
        assert [t.shape[0] for t in na[:4]] == [na[4]] * 4 and [o.shape[0] for o in out] == [4 * pa[4]] * 4     # ... its leading rows
    last = levels[2][2]
    assert all(last[k] is None for k in ("d_out_rays", "d_out_weights", "d_out_pixels", "d_out_ids", "d_out_count", "d_out_lowres"))


@pytest.mark.parametrize("environment,image", [(dict(bg_color=(0.1, 0.2, 0.3)), False), (dict(pixels=np.zeros((24, 48, 3), np.float32)), True)])
def test_the_lowres_byte_goes_from_level_to_level(environment, image):
    """With an environment, image or colour, every level with children writes one byte per child next to the queue, and the next
    level reads its leading rows as d_lowres; the eye rays have none.  Mixed kinds under an IMAGE are accepted (the batched
    route's ValueError does not apply) and MR_ENV_LOWRES is never set: the bytes say it."""
    sc, _, _ = run("table", depth=2, path_kinds=7, environment=environment, **PATH)
    assert [c[0] for c in sc.calls] == ["set_environment", "get_environment", "set_lights"] + [NAME] * 3
    assert all(c[2]["environment"] is True and not c[2]["flags"] & binding.MR_ENV_LOWRES for c in sc.calls[3:])
    assert sc.raw[0][1]["d_lowres"] is None and sc.raw[2][1]["d_out_lowres"] is None
    for (pa, pkw), (na, nkw) in zip(sc.raw, sc.raw[1:]):
        low = pkw["d_out_lowres"]
        assert low.dtype == torch.uint8 and low.shape[0] == 4 * pa[4]
        assert nkw["d_lowres"].data_ptr() == low.data_ptr() and nkw["d_lowres"].shape[0] == na[4]
    with pytest.raises(ValueError) as e:                        # the batched route still refuses the mixture under an image
        run("table", image=True, depth=2, lights=LIGHTS, path_tracing=True, path_kinds=7, environment=True)
    assert "Ray::random" in str(e.value)
    sc, _, _ = run("plain", image=image, depth=1, environment=True, **PATH)
    assert [c[0] for c in sc.calls] == ["get_environment", "set_lights"] + [NAME] * 2


@pytest.mark.parametrize("scene", ["table", "procedural"])
def test_photon_maps_follow_each_level(scene):
    """each level is followed by gather_level on the hit records the level wrote (level 0: the renderer's d_hits), with the
    level's queue, and with the level's normal buffer on a procedural scene only"""
    sc, _, per_level = run(scene, depth=2, photon_maps=(FakeMap(), None), nphotons=50, max_dist=2.0, **PATH)
    assert [c[0] for c in sc.calls] == ["set_lights"] + [NAME, "gather_level"] * 3
    assert len(per_level) == 3
    for k in range(3):
        (_, la, lkw), (_, ga, gkw) = sc.calls[1 + 2 * k], sc.calls[2 + 2 * k]
        assert lkw["d_hits"] is not None and ga[3] == lkw["d_hits"] and ga[2] == la[0] and ga[4] == la[4]
        assert (label(sc, lkw["d_hits"]) == "d_hits") == (k == 0)
        assert gkw["d_weights"] == la[1] and gkw["d_pixels"] == la[2] and gkw["nphotons"] == 50 and gkw["max_dist"] == 2.0
        if scene == "procedural":
            assert lkw["d_normal"] is not None and gkw["d_normal"] == lkw["d_normal"]
        else:
            assert lkw["d_normal"] is None and gkw["d_normal"] is None


@pytest.mark.parametrize("kw,square,word", [
    (dict(group_octants=True), False, "group_octants"), (dict(surface_children=False), False, "surface_children=False"),
    (dict(), True, "square lights"), (dict(path_tracing=False), False, "path_tracing=True")])
def test_what_the_route_refuses(kw, square, word):
    with pytest.raises(ValueError) as e:
        run("plain", square=square, depth=2, **dict(PATH, **kw))
    assert word in str(e.value) and "fused=\"lights_path\"" in str(e.value)


def test_it_needs_a_light_list():
    with pytest.raises(ValueError) as e:
        run("plain", depth=2, fused="lights_path", path_tracing=True)
    assert "lights=[...]" in str(e.value) and "fused=\"lights_path\"" in str(e.value)


def test_the_other_routes_never_take_it():
    """fused=True / "auto" / False / "lights" launch what they launched before: no trace_level_lights_path; and fused="lights"
    keeps refusing path_tracing"""
    for fused in (False, True, "auto"):
        sc, _, _ = run("plain", depth=2, fused=fused)
        assert NAME not in [c[0] for c in sc.calls]
    sc, _, _ = run("plain", depth=2, fused="lights", lights=LIGHTS)
    assert [c[0] for c in sc.calls][:2] == ["set_lights", "trace_level_lights"] and NAME not in [c[0] for c in sc.calls]
    with pytest.raises(ValueError) as e:
        run("plain", depth=2, fused="lights", lights=LIGHTS, path_tracing=True)
    assert "path_tracing" in str(e.value) and "fused=\"lights\"" in str(e.value)
