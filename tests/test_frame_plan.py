"""FrameRenderer.render_specular's launch sequence, pinned on torch's CPU device: a recording stand-in for binding.Scene
takes every call the driver makes -- name, arguments, which buffer goes where -- and moves the counters as the launch
would.  The record of every case below is compared with tests/golden/render_specular_calls.json, which holds per case
the inputs, the result (or the exception), the call names and the SHA-256 of the full record's canonical JSON.

    python tests/test_frame_plan.py --write      regenerates the golden file from the code as it stands
"""
import hashlib
import itertools
import json
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if os.path.join(ROOT, "cse168-raytracer_amd") not in sys.path:
    sys.path.insert(0, os.path.join(ROOT, "cse168-raytracer_amd"))

from miro_amd import binding, frame  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "render_specular_calls.json")
W, H, SPP = 8, 4, 2
DESC = dict(eye=(0.0, 2.0, 6.0), lookat=(0.0, 1.0, 0.0), up=(0.0, 1.0, 0.0), fov=45.0, light=(1.0, 4.0, 2.0), wattage=300.0)
LIGHTS = [dict(position=(1.0, 4.0, 2.0), wattage=200.0),
          dict(position=(0.0, 5.0, 0.0), normal=(0.0, -1.0, 0.0), color=(1.0, 0.9, 0.8), wattage=100.0, radius=0.5)]
SQUARE = [dict(position=(0.0, 4.5, 0.0), wattage=150.0, dimensions=(1.0, 0.5))]


class FakeMap:
    """stands for a binding.PhotonMap: recorded by type name"""


# position of n and of the counter that the launch writes, per binding.Scene's signatures
HIT_COUNTERS = {"shade_lights": 2, "shade_lights_surface": 4, "shade_square_lights": 4, "shade_square_lights_surface": 6}
GENERATORS = {"gen_secondary_rays": (4, 8), "gen_path_rays": (5, 10), "gen_path_rays_surface": (7, 12)}


class RecordingScene:
    """device, n_textures, procedural; every other attribute is a method that appends (name, args, kwargs) to `calls` and
    then does to the counters what the launch would: `hit` of the rays hit something, `child` of them have a child (integer
    ratios).  Every tensor seen stays alive, so that no address comes back for another buffer."""

    def __init__(self, n_textures, procedural, hit, child, image):
        self.device, self.n_textures, self.procedural = 0, n_textures, procedural
        self.hit, self.child, self.image = hit, child, image
        self.calls, self.labels, self.keep = [], {}, []

    def register(self, t, name):
        self.keep.append(t)
        self.labels.setdefault((t.data_ptr(), tuple(t.shape), str(t.dtype)), name)

    def encode(self, v):
        if isinstance(v, torch.Tensor):
            self.register(v, len(self.labels))
            key = (v.data_ptr(), tuple(v.shape), str(v.dtype))
            return ["tensor", self.labels[key], list(v.shape), str(v.dtype)]
        if isinstance(v, (list, tuple)):
            return [self.encode(x) for x in v]
        if isinstance(v, dict):
            return {str(k): self.encode(x) for k, x in v.items()}
        if v is None or isinstance(v, (bool, int, float, str)):
            return v
        return {"type": type(v).__name__}

    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)

        def call(*args, **kw):
            self.calls.append([name, self.encode(args), self.encode(kw)])
            return self.launch(name, args, kw)
        return call

    def part(self, n, ratio):
        return n * ratio[0] // ratio[1]

    def launch(self, name, a, kw):
        if name == "trace_level":
            n = a[4]
            kw["d_counts"][0] += n
            kw["d_counts"][1] += self.part(n, self.hit)
            if kw["d_out_count"] is not None:
                kw["d_out_count"][0] = self.part(n, self.child)
        elif name == "gen_shadow_rays":
            a[6][0] = self.part(a[2], self.hit)
        elif name in HIT_COUNTERS:
            kw["d_counts"][0] += self.part(a[HIT_COUNTERS[name]], self.hit)
        elif name in GENERATORS:
            n_at, count_at = GENERATORS[name]
            a[count_at][0] = self.part(a[n_at], self.child)
        elif name == "set_environment":
            self.image = kw.get("pixels") is not None
        elif name == "get_environment":
            return ("image", 1.0) if self.image else (None, 0.0)
        return None


SCENES = {"plain": (0, False), "table": (2, False), "procedural": (2, True)}
PATH7 = dict(depth=2, path_tracing=True, path_seed=5, path_kinds=7)
CALLS = [
    ("depth2", dict(depth=2), {}),
    ("fused", dict(depth=2, fused=True), {}),
    ("auto_half_hit", dict(depth=2, fused="auto"), dict(hit=(1, 2))),
    ("auto_all_hit", dict(depth=2, fused="auto"), dict(hit=(1, 1))),
    ("lights", dict(depth=2, lights=LIGHTS), {}),
    ("grouped", dict(depth=2, group_octants=True), {}),
    ("grouped_fused", dict(depth=2, group_octants=True, fused=True), {}),
    ("path7", dict(PATH7), {}),
    ("path7_surface_children", dict(PATH7, surface_children=True), {}),
    ("path7_plain_children_lights", dict(PATH7, surface_children=False, lights=LIGHTS), {}),
    ("env_dict", dict(depth=2, environment=dict(bg_color=(0.1, 0.2, 0.3))), {}),
    ("env_true_diffuse", dict(depth=2, environment=True, path_tracing=True, path_kinds=binding.MR_PATH_DIFFUSE), dict(image=True)),
    ("env_image_mixed", dict(PATH7, environment=dict(pixels=[[[1.0, 1.0, 1.0]]], rotation=(0.5, 0.0))), {}),
    ("photon_lights", dict(depth=2, photon_maps=(FakeMap(), FakeMap()), nphotons=50, max_dist=2.0, lights=LIGHTS), {}),
    ("photon_fused", dict(depth=2, photon_maps=(FakeMap(), None), fused=True), {}),
    ("lights_fused", dict(depth=2, lights=LIGHTS, fused=True), {}),
    ("stream0", dict(depth=2, stream=0), {}),
    ("depth0", dict(depth=0), {}),
    ("no_rays", dict(depth=2), dict(bands=[])),
    ("dies_out", dict(depth=2), dict(child=(0, 1))),
]
CASES = {"%s-%s-%s" % (s, "square" if sq else "nosquare", name): (s, sq, kw, extra)
         for (s, sq), (name, kw, extra) in itertools.product(itertools.product(SCENES, (False, True)), CALLS)}


def run_case(case):
    """the full record of one case: inputs, calls, and per_level or the exception"""
    s, square, kw, extra = CASES[case]
    sc = RecordingScene(*SCENES[s], hit=extra.get("hit", (3, 4)), child=extra.get("child", (1, 2)), image=extra.get("image", False))
    fr = frame.FrameRenderer(sc, DESC, W, H, spp=SPP, bands=extra.get("bands"), device=torch.device("cpu"),
                             square_lights=SQUARE if square else None, square_samples=4 if square else 1)
    for name, t in sorted(vars(fr).items()):                    # the renderer's own buffers go by name
        if isinstance(t, torch.Tensor):
            sc.register(t, name)
    rec = {"inputs": dict(scene=s, square_lights=square, kwargs=sc.encode(kw), **sc.encode(extra))}
    try:
        rec["per_level"] = sc.encode(fr.render_specular(**kw))
    except (ValueError, TypeError) as e:
        rec["raises"] = [type(e).__name__, str(e)]
    rec["calls"] = sc.calls
    return rec


def summary(rec):
    """what the golden file keeps of a record"""
    out = {k: rec[k] for k in ("inputs", "per_level", "raises") if k in rec}
    out["calls"] = [c[0] for c in rec["calls"]]
    out["sha256"] = hashlib.sha256(json.dumps(rec, sort_keys=True, separators=(",", ":")).encode()).hexdigest()
    return out


def write_golden():
    lines = ["%s: %s" % (json.dumps(c), json.dumps(summary(run_case(c)), sort_keys=True)) for c in CASES]
    with open(GOLDEN, "w") as fh:
        fh.write("{\n" + ",\n".join(lines) + "\n}\n")


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as fh:
        return json.load(fh)


def test_golden_holds_these_cases(golden):
    assert list(golden) == list(CASES)
    refused = [c for c, g in golden.items() if "raises" in g]
    assert {golden[c]["raises"][0] for c in refused} == {"ValueError", "TypeError"}
    assert sum(len(g["calls"]) for g in golden.values()) > 1000


@pytest.mark.parametrize("case", list(CASES))
def test_launch_sequence(case, golden, tmp_path):
    rec = run_case(case)
    got, want = summary(rec), golden[case]
    if got != want:
        path = tmp_path / (case + ".json")
        path.write_text(json.dumps(rec, indent=1, sort_keys=True))
        names = "call names %s" % ("agree" if got["calls"] == want["calls"] else "differ: %s, golden %s" % (got["calls"], want["calls"]))
        result = {k: (got.get(k), want.get(k)) for k in ("per_level", "raises") if got.get(k) != want.get(k)}
        raise AssertionError("%s: %s; result (got, golden) %s; full record in %s" % (case, names, result or "agrees", path))


def test_record_is_repeatable():
    for case in ("procedural-square-path7", "plain-nosquare-auto_half_hit", "table-square-photon_lights"):
        assert json.dumps(run_case(case), sort_keys=True) == json.dumps(run_case(case), sort_keys=True)


if __name__ == "__main__":
    if sys.argv[1:] != ["--write"]:
        sys.exit(__doc__)
    write_golden()
    print("wrote %s: %d cases, %d calls" % (GOLDEN, len(CASES), sum(len(run_case(c)["calls"]) for c in CASES)))
