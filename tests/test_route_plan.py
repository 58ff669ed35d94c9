"""FrameRenderer.render_specular's 14 string routes (fused="lights" ... "device_lens_photons_path"), pinned on torch's CPU device
the way tests/test_frame_plan.py pins the other values of `fused`: its recording stand-in, extended by the launches and the two
size queries these routes make, takes every call the driver makes, and the record of every case below -- the valid frame of each
route on each scene, that frame with one thing changed, pairs of such changes on two routes, and values of `fused` that are no
route -- is compared with tests/golden/render_specular_routes.json (inputs, result or exception with its full text, call names,
SHA-256 of the full record).

    python tests/test_route_plan.py --write [FILE]     regenerates the golden file (or FILE) from the code as it stands
"""
import itertools
import json
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_frame_plan import DESC, LIGHTS, SCENES, SQUARE, FakeMap, RecordingScene, summary  # noqa: E402
from test_recursion_device_plan import workspace as queues  # noqa: E402
from test_recursion_photons_plan import workspace as photons_workspace  # noqa: E402

from miro_amd import binding, frame  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "render_specular_routes.json")
W, H, SPP = 8, 4, 2
PATH = binding.MR_LEVEL_PATH
LENS = dict(aperture=0.1, focus_plane=4.0)
ROUTES = ["lights", "lights_path", "frame_lights", "frame_lights_path", "device_lights", "device_lights_path", "device_photons",
          "device_photons_path", "frame_lens", "frame_lens_path", "device_lens", "device_lens_path", "device_lens_photons",
          "device_lens_photons_path"]
PAIRED = ["frame_lights", "device_lens_photons_path"]
VALID_SCENES = list(SCENES)
# the golden stays under 256 KB: the pairs leave out the changes that concern no check (with them the file is 300 KB)
UNPAIRED = ["depth0", "no_rays", "dies_out", "small_queue"]


class Recorder(RecordingScene):
    """RecordingScene that answers the two workspace queries with the headers' formulas and moves the counters of the level-0
    frames, the level calls and the one-call recursions: `hit` of a level's rays cast a shadow ray (and are queries), `child` of
    them have a child, a device queue holds queue_capacity"""

    def launch(self, name, a, kw):
        if name == "recursion_workspace_bytes":
            return 0 if a[0] == 0 else queues(a[1], kw["children"] == PATH, kw["environment"])
        if name == "recursion_photons_workspace_bytes":
            return photons_workspace((kw["y1"] - kw["y0"]) * a[1] * kw["spp"], a[3], a[4], kw["children"] == PATH, kw["environment"])
        if name in ("render_recursion", "render_recursion_lens", "render_recursion_photons", "render_recursion_photons_lens"):
            counts, depth = a[4], a[5]
            n = (kw["y1"] - kw["y0"]) * a[1] * kw["spp"]
            counts.zero_()
            for level in range(depth + 1):
                counts[level, 0], counts[level, 1] = n, self.part(n, self.hit)
                if "photons" in name:
                    counts[level, 6] = self.part(n, self.hit)
                if level < depth:
                    counts[level, 5] = self.part(n, self.child)
                n = min(int(counts[level, 5]), kw["queue_capacity"])
            return None
        if name in ("render_level_lights", "render_level_lights_lens"):
            n = (kw["y1"] - kw["y0"]) * a[1] * kw["spp"]
        elif name == "trace_level_lights":
            n = a[3]
        elif name == "trace_level_lights_path":
            n = a[4]
        else:
            return super().launch(name, a, kw)          # gather_level among them: it moves no counter the driver reads
        kw["d_counts"][0] += n
        kw["d_counts"][1] += self.part(n, self.hit)
        if kw["d_out_count"] is not None:
            kw["d_out_count"][0] = self.part(n, self.child)
        return None


MAPS = (FakeMap(), FakeMap())
DROP = "<dropped>"                                      # a changed keyword that is withheld, not given another value
# the inputs of a record name these three (the golden stays small); the calls that receive them are recorded in full
NAMED = {id(LIGHTS): "LIGHTS", id(MAPS): "MAPS", id(LENS): "LENS"}


def is_path(route):
    return route.endswith("_path")


def is_lens(route):
    return "_lens" in route


def is_device(route):
    return route.startswith("device_")


def maps_inside(route):
    return "photons" in route


def valid(route):
    """(the renderer's options, render_specular's keywords) of the route's valid frame at depth 2"""
    kw = dict(depth=2, lights=LIGHTS, fused=route)
    if is_path(route):
        kw.update(path_tracing=True, path_seed=5, path_kinds=7)
    if maps_inside(route):
        kw.update(photon_maps=MAPS)
    return (dict(lens=LENS) if is_lens(route) else {}), kw


def changes(route):
    """name -> (changed renderer options, changed keywords): the one-thing perturbations of valid(route)"""
    _, kw = valid(route)
    toggled = DROP if "photon_maps" in kw else MAPS
    out = {
        "no_lights": ({}, dict(lights=DROP)),
        "path_flipped": ({}, dict(path_tracing=not is_path(route))),
        "surface_children": ({}, dict(surface_children=True)),
        "plain_children": ({}, dict(surface_children=False)),
        "grouped": ({}, dict(group_octants=True)),
        "square": (dict(square=True), {}),
        "two_bands": (dict(bands=[(0, 2), (3, 4)]), {}),
        "lens_flipped": (dict(lens=None if is_lens(route) else LENS), {}),
        "maps_flipped": ({}, dict(photon_maps=toggled)),
        "no_resident": (dict(resident=False), {}),
        "no_resident_maps_flipped": (dict(resident=False), dict(photon_maps=toggled)),
        "env_image_kinds7": ({}, dict(environment=dict(pixels=[[[1.0, 1.0, 1.0]]], rotation=(0.5, 0.0)), path_kinds=7)),
        "stream0": ({}, dict(stream=0)),
        "depth0": ({}, dict(depth=0)),
        "no_rays": (dict(bands=[]), {}),
        "dies_out": (dict(child=(0, 1)), {}),
    }
    # lens eye rays come in image order: FrameRenderer refuses lens with tiled=True, so on a lens route the flag is set afterwards
    out["tiled"] = (dict(tiled_afterwards=True) if is_lens(route) else dict(tiled=True), {})
    if is_device(route):
        out["small_queue"] = ({}, dict(queue_capacity=10))      # level 0 of 64 samples emits 32 children
    return out


def merged(base, *deltas):
    out = dict(base)
    for d in deltas:
        out.update(d)
    return {k: v for k, v in out.items() if v is not DROP}


def make_cases():
    cases = {}
    for route, scene in itertools.product(ROUTES, VALID_SCENES):
        make, kw = valid(route)
        cases["valid-%s-%s" % (route, scene)] = (scene, make, kw)
        cases["valid-%s-%s-env" % (route, scene)] = (scene, make, dict(kw, environment=dict(bg_color=(0.1, 0.2, 0.3))))
        if not is_device(route):                                # the routes that take their maps from the caller
            cases["valid-%s-%s-maps" % (route, scene)] = (scene, make, dict(kw, photon_maps=MAPS))
    for route in ROUTES:
        make, kw = valid(route)
        for name, (dm, dk) in changes(route).items():
            cases["one-%s-%s" % (route, name)] = ("plain", merged(make, dm), merged(kw, dk))
    for route in PAIRED:
        make, kw = valid(route)
        paired = [(n, c) for n, c in changes(route).items() if n not in UNPAIRED]
        for (na, (ma, ka)), (nb, (mb, kb)) in itertools.combinations(paired, 2):
            if set(ma) & set(mb) or set(ka) & set(kb):
                continue                                        # the two change the same thing
            cases["two-%s-%s-%s" % (route, na, nb)] = ("plain", merged(make, ma, mb), merged(kw, ka, kb))
    for fused, lights in itertools.product(("bogus", 1), (False, True)):
        cases["other-%s-%s" % (fused, "lights" if lights else "nolights")] = \
            ("plain", {}, dict(depth=2, fused=fused, **(dict(lights=LIGHTS) if lights else {})))
    return cases


CASES = make_cases()


def run_case(case):
    """the full record of one case: inputs, calls, and per_level or the exception"""
    s, make, kw = CASES[case]
    sc = Recorder(*SCENES[s], hit=(3, 4), child=make.get("child", (1, 2)), image=False)
    square = make.get("square", False)
    named = lambda d: {k: NAMED.get(id(v), v) for k, v in d.items()}                                       # noqa: E731
    rec = {"inputs": dict(scene=s, renderer=sc.encode(named(make)), kwargs=sc.encode(named(kw)))}
    try:                                                        # the renderer itself refuses a lens with tiled=True
        fr = frame.FrameRenderer(sc, DESC, W, H, spp=SPP, bands=make.get("bands"), device=torch.device("cpu"), tiled=make.get("tiled"),
                                 lens=make.get("lens"), square_lights=SQUARE if square else None, square_samples=4 if square else 1,
                                 resident_rays=make.get("resident", True))
        if make.get("tiled_afterwards"):
            fr.tiled = True
        for name, t in sorted(vars(fr).items()):                # the renderer's own buffers go by name
            if isinstance(t, torch.Tensor):
                sc.register(t, name)
        rec["per_level"] = sc.encode(fr.render_specular(**kw))
    except (ValueError, TypeError, RuntimeError) as e:
        rec["raises"] = [type(e).__name__, str(e)]
    rec["calls"] = sc.calls
    return rec


def write_golden(path=GOLDEN):
    lines = ["%s: %s" % (json.dumps(c), json.dumps(summary(run_case(c)), sort_keys=True)) for c in CASES]
    with open(path, "w") as fh:
        fh.write("{\n" + ",\n".join(lines) + "\n}\n")


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as fh:
        return json.load(fh)


def test_golden_holds_these_cases(golden):
    """the golden's cases are CASES; no route is missing from the valid frames, the one-thing changes or (the two paired routes) the
    pairs; every route has a case that ends in per_level; all three exception types occur; the file stays under 256 KB"""
    assert list(golden) == list(CASES)
    for route in ROUTES:
        assert {"valid-%s-%s%s" % (route, s, v) for s in VALID_SCENES for v in ("", "-env")} <= set(CASES)
        ones = [c for c in CASES if c.startswith("one-%s-" % route)]
        assert len(ones) >= 17 and all(CASES[c][2].get("fused", route) == route for c in ones)
        ran = [c for c, g in golden.items() if g["inputs"]["kwargs"].get("fused") == route and "per_level" in g]
        assert ran and any(golden[c]["per_level"] for c in ran), route
    for route in PAIRED:
        assert sum(c.startswith("two-%s-" % route) for c in CASES) > 80
    assert {c.split("-")[1] for c in CASES if c.startswith("other-")} == {"bogus", "1"}
    assert {g["raises"][0] for g in golden.values() if "raises" in g} == {"ValueError", "TypeError", "RuntimeError"}
    assert sum(len(g["calls"]) for g in golden.values()) > 500
    assert os.path.getsize(GOLDEN) < 256 * 1024


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
    for case in ("valid-device_lens_photons_path-procedural-env", "valid-frame_lights-table-maps", "one-lights_path-env_image_kinds7"):
        assert json.dumps(run_case(case), sort_keys=True) == json.dumps(run_case(case), sort_keys=True)


if __name__ == "__main__":
    if sys.argv[1:2] != ["--write"] or len(sys.argv) > 3:
        sys.exit(__doc__)
    write_golden(*sys.argv[2:])
    print("wrote %s: %d cases, %d calls" % ((sys.argv[2:] or [GOLDEN])[0], len(CASES), sum(len(run_case(c)["calls"]) for c in CASES)))
