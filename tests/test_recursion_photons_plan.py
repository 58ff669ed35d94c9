"""mr_render_recursion_photons without a GPU (include/miro_hip_recursion_photons.h, csrc/mr_gather_queued.hip): the two symbols and
their list, the workspace formula, the argument errors before any device call, what render_specular(fused="device_photons" |
"device_photons_path") hands to the library -- recorded by the stand-in scene of tests/test_frame_plan.py, extended by the one call
this route makes --, what the route refuses, that fused="device_lights[_path]" with photon_maps is refused as before, and the
unit's kernels against their golden record."""
import ctypes as C
import json
import os
import re
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kernel_budget  # noqa: E402
from miro_amd import binding, frame  # noqa: E402
from test_frame_lights import frame_desc  # noqa: E402
from test_frame_plan import CASES, DESC, GOLDEN, LIGHTS, SCENES, SQUARE, FakeMap, RecordingScene  # noqa: E402
from test_recursion_device_plan import rdesc, workspace as queues  # noqa: E402

NAMES = ["mr_render_recursion_photons_workspace", "mr_render_recursion_photons"]
W, H, SPP = 16, 8, 2
N = W * H * SPP
SPECULAR, PATH = binding.MR_LEVEL_SPECULAR, binding.MR_LEVEL_PATH


def tiled_desc():
    fd = frame_desc(binding)
    fd.tiled = 1
    return fd


def header(name):
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", name)).read(), flags=re.S)


def test_the_two_symbols_are_exported_declared_and_bound(miro):
    """Fails on the parent commit: the symbols, the header and the sixth list are this feature's.  The older five lists are as they
    were, and miro_hip.h alone reaches the new header (miro_hip_recursion.h's last line, below its declarations)."""
    others = ("miro_hip.h", "miro_hip_surface.h", "miro_hip_frame.h", "miro_hip_render.h", "miro_hip_recursion.h")
    for name in NAMES:
        declared = lambda h: re.search(r"\bmr_status\s+%s\s*\(" % name, header(h)) is not None              # noqa: E731
        assert hasattr(miro.lib(), name) and getattr(miro.lib(), name).restype is C.c_int32
        assert declared("miro_hip_recursion_photons.h") and not any(declared(h) for h in others)
        assert name not in (binding.RECURSION_SYMBOLS + binding.RENDER_SYMBOLS + binding.FRAME_SYMBOLS + binding.SURFACE_SYMBOLS +
                            miro.EXPORTED_SYMBOLS)
    assert binding.RECURSION_PHOTONS_SYMBOLS == NAMES
    assert binding.RECURSION_SYMBOLS == ["mr_render_recursion_workspace", "mr_render_recursion"]
    assert len(miro.EXPORTED_SYMBOLS) == 69 and len(binding.SURFACE_SYMBOLS) == 9 and len(binding.FRAME_SYMBOLS) == 3
    assert binding.RENDER_SYMBOLS == ["mr_render_level_lights"]
    top = open(os.path.join(ROOT, "include", "miro_hip.h")).read()
    assert top.rstrip().endswith('#include "miro_hip_render.h"\n#endif /* MIRO_HIP_H */')
    assert '#include "miro_hip_recursion.h"' in header("miro_hip_render.h")
    rec = open(os.path.join(ROOT, "include", "miro_hip_recursion.h")).read()
    assert rec.rstrip().endswith('#endif /* MIRO_HIP_RECURSION_H */\n#include "miro_hip_recursion_photons.h"')
    assert hasattr(miro.Scene, "render_recursion_photons") and hasattr(miro.Scene, "recursion_photons_workspace_bytes")


def workspace(samples, depth, capacity, path, env):
    """the header's formula: mr_render_recursion_workspace's two queues, then for M = max(samples, capacity if depth >= 1) rays 16 M
    bytes of hit records, 12 M of normals and 48 M of scratch, each rounded up to 16 bytes"""
    up = lambda v: (v + 15) // 16 * 16                                                                       # noqa: E731
    m = max(samples, capacity if depth >= 1 else 0)
    return (queues(capacity, path, env) if depth >= 1 else 0) + up(16 * m) + up(12 * m) + up(48 * m)


def test_workspace_bytes_is_the_formula(miro):
    """capacities 1, 100, 257, 4099 below and above the window's samples (16 x 8 x 2 = 256 and 3 x 5 x 1 = 15), specular and path,
    with and without environment, depth 0"""
    L = miro.lib()
    out = C.c_uint64(12345)
    windows = [(frame_desc(binding, W=W, H=H, spp=SPP), N), (frame_desc(binding, W=3, H=H, spp=1, y0=2, y1=7), 15)]
    for fd, samples in windows:
        for capacity in (1, 100, 257, 4099):
            for children in (SPECULAR, PATH):
                for env in (0, 1):
                    for depth in (3, 1, 0):
                        rd = rdesc(depth, children, env, capacity=capacity)
                        assert L.mr_render_recursion_photons_workspace(C.byref(fd), C.byref(rd), C.byref(out)) == binding.MR_OK
                        assert out.value == workspace(samples, depth, capacity, children == PATH, env), (samples, capacity, children, env, depth)
    assert workspace(N, 3, 100, False, 0) == queues(100, False, 0) + 76 * N          # the samples exceed the capacity
    assert workspace(N, 3, 257, False, 0) == queues(257, False, 0) + 16 * 257 + 3088 + 12336                 # and here they do not
    fd = windows[0][0]
    out.value = 777
    bad = [("NULL", (None, C.byref(rdesc()), C.byref(out))), ("NULL", (C.byref(fd), None, C.byref(out))),
           ("NULL", (C.byref(fd), C.byref(rdesc()), None)), ("reserved", (C.byref(fd), C.byref(rdesc(reserved=0)), C.byref(out))),
           ("depth", (C.byref(fd), C.byref(rdesc(depth=65)), C.byref(out))),
           ("children", (C.byref(fd), C.byref(rdesc(children=0)), C.byref(out))),
           ("queue_capacity", (C.byref(fd), C.byref(rdesc(capacity=0)), C.byref(out))),
           ("queue_capacity", (C.byref(fd), C.byref(rdesc(capacity=1 << 31)), C.byref(out))),
           ("spp", (C.byref(frame_desc(binding, spp=3)), C.byref(rdesc()), C.byref(out))),
           ("empty image", (C.byref(frame_desc(binding, W=0)), C.byref(rdesc()), C.byref(out))),
           ("tiled", (C.byref(tiled_desc()), C.byref(rdesc()), C.byref(out)))]
    for word, args in bad:
        assert L.mr_render_recursion_photons_workspace(*args) == binding.MR_ERR_INVALID, word
        msg = L.mr_last_error()
        assert word.encode() in msg and b"mr_render_recursion_photons_workspace" in msg, (word, msg)
    assert out.value == 777                                                       # a refused call writes nothing


def test_argument_errors_come_before_the_scene_and_the_device(miro):
    """Every MR_ERR_INVALID case on a host_only one-triangle scene with two unbalanced maps: answered from the arguments alone, under
    this call's name, before any device call and before a map's state is read, so "no HIP device", "host_only" and "balanced" may
    not be what comes back.  mr_render_recursion's cases first, then this call's.  Then MR_ERR_STATE for that scene."""
    L = miro.lib()
    s = miro.Scene()
    s.add_triangle([0, 0, 0, 1, 0, 0, 0, 1, 0], [0, 0, 1] * 3)
    s.set_lights([dict(position=(0, 1, 0), wattage=5.0)])
    s.build(4, host_only=True)
    g, c = miro.PhotonMap(64), miro.PhotonMap(64)
    p = lambda a: C.c_void_p(a)                                                   # noqa: E731
    fd, ok = frame_desc(binding), rdesc()
    samples = fd.W * (fd.y1 - fd.y0) * fd.spp
    need = workspace(samples, 3, 100, False, 0)
    base = dict(scene=s.h, g=g.h, c=c.h, dist=1e10, k=50, rgb=p(8192), ws=p(1 << 20), bytes=need, counts=p(1 << 16))

    def call(fd, rd, **kw):
        a = dict(base, **kw)
        st = L.mr_render_recursion_photons(a["scene"], C.byref(fd) if fd is not None else None, C.byref(rd) if rd is not None else None,
                                           a["g"], a["c"], a["dist"], a["k"], a["rgb"], a["ws"], a["bytes"], a["counts"], None)
        return st, L.mr_last_error()

    invalid = [
        ("NULL", call(fd, ok, scene=None)), ("NULL", call(None, ok)), ("NULL", call(fd, ok, rgb=None)),
        ("empty image", call(frame_desc(binding, W=0), ok)),
        ("spp", call(frame_desc(binding, spp=3), ok)),
        ("flags", call(frame_desc(binding, flags=binding.MR_TRACE_ANY), ok)), ("flags", call(frame_desc(binding, flags=1 << 30), ok)),
        ("aligned", call(fd, ok, rgb=p(8194))), ("aligned", call(fd, ok, counts=p((1 << 16) + 4))),
        ("NULL", call(fd, None)), ("d_level_counts", call(fd, ok, counts=None)),
        ("depth", call(fd, rdesc(depth=65))),
        ("children", call(fd, rdesc(children=0))), ("children", call(fd, rdesc(children=7))),
        ("environment", call(fd, rdesc(environment=2))),
        ("path_kinds", call(fd, rdesc(children=PATH, kinds=0))), ("path_kinds", call(fd, rdesc(children=PATH, kinds=8))),
        ("reserved", call(fd, rdesc(reserved=0))), ("reserved", call(fd, rdesc(reserved=4))),
        ("queue_capacity", call(fd, rdesc(capacity=0))), ("queue_capacity", call(fd, rdesc(capacity=1 << 31))),
        ("workspace", call(fd, ok, ws=None)), ("workspace", call(fd, ok, ws=p((1 << 20) + 8))),
        ("workspace", call(fd, rdesc(depth=0, children=0, capacity=0), ws=None, bytes=0)),                   # needed at depth 0 too
        ("workspace_bytes", call(fd, ok, bytes=need - 1)), ("workspace_bytes", call(fd, ok, bytes=0)),
        ("workspace_bytes", call(fd, ok, bytes=queues(100, False, 0))),                                      # mr_render_recursion's size
        ("workspace_bytes", call(fd, rdesc(children=PATH), bytes=need)),
        # this call's own
        ("both NULL", call(fd, ok, g=None, c=None)),
        ("nphotons", call(fd, ok, k=0)), ("nphotons", call(fd, ok, k=513)),
        ("max_dist", call(fd, ok, dist=0.0)), ("max_dist", call(fd, ok, dist=-1.0)), ("max_dist", call(fd, ok, dist=float("nan"))),
        ("tiled", call(tiled_desc(), ok)),
    ]
    for word, (st, msg) in invalid:
        assert st == binding.MR_ERR_INVALID, (word, st, msg)
        assert word.encode() in msg and b"mr_render_recursion_photons" in msg, (word, msg)
        assert b"HIP device" not in msg and b"host_only" not in msg and b"balanced" not in msg, (word, msg)
    for good in (call(fd, ok), call(fd, ok, c=None), call(fd, ok, g=None, k=512),
                 call(fd, rdesc(depth=0, children=0, capacity=0), bytes=workspace(samples, 0, 0, False, 0))):
        st, msg = good                                                            # then the scene's state: never a CPU path
        assert st == binding.MR_ERR_STATE and (b"CPU" in msg or b"device" in msg) and b"HIP device" not in msg, msg
    unbuilt = miro.Scene()
    unbuilt.add_triangle([0, 0, 0, 1, 0, 0, 0, 1, 0], [0, 0, 1] * 3)
    st, msg = call(fd, ok, scene=unbuilt.h)
    assert st == binding.MR_ERR_STATE and b"mr_bvh_build" in msg, msg
    st, msg = call(fd, ok, scene=unbuilt.h, k=0)
    assert st == binding.MR_ERR_INVALID and b"nphotons" in msg                    # still the arguments first
    assert s.info().n_triangles == 1 and g.count() == 0                           # the refused calls left scene and maps alone


# ---- the driver, recorded -----------------------------------------------------------------------------------------------------
class Recorder(RecordingScene):
    """RecordingScene that answers recursion_photons_workspace_bytes with the header's formula and does to d_level_counts what
    mr_render_recursion_photons would: `hit` of a level's rays cast a shadow ray and are queries, `child` of them have a child"""

    def launch(self, name, a, kw):
        if name == "recursion_photons_workspace_bytes":
            return workspace((kw["y1"] - kw["y0"]) * a[1] * kw["spp"], a[3], a[4], kw["children"] == PATH, kw["environment"])
        if name != "render_recursion_photons":
            assert name not in ("render_recursion", "render_level_lights", "trace_level_lights", "trace_level_lights_path", "gather_level",
                                "gen_eye_rays"), name
            return super().launch(name, a, kw)
        counts, depth = a[4], a[5]
        n = (kw["y1"] - kw["y0"]) * a[1] * kw["spp"]
        counts.zero_()
        for level in range(depth + 1):
            counts[level, 0], counts[level, 1], counts[level, 6] = n, self.part(n, self.hit), self.part(n, self.hit)
            if level < depth:
                counts[level, 5] = self.part(n, self.child)
            n = min(int(counts[level, 5]), kw["queue_capacity"])
        return None


def render(scene="plain", tiled=None, bands=None, lens=None, square=False, resident=True, child=(1, 2), frames=1, **kw):
    sc = Recorder(*SCENES[scene], hit=(3, 4), child=child, image=False)
    fr = frame.FrameRenderer(sc, DESC, W, H, spp=SPP, bands=bands, device=torch.device("cpu"), tiled=tiled, lens=lens,
                             square_lights=SQUARE if square else None, resident_rays=resident)
    for name, t in sorted(vars(fr).items()):                    # the renderer's own buffers go by name
        if isinstance(t, torch.Tensor):
            sc.register(t, name)
    per_level = [fr.render_specular(**kw) for _ in range(frames)]
    return sc, fr, per_level[-1]


def names(sc):
    return [c[0] for c in sc.calls]


MAPS = (FakeMap(), FakeMap())


@pytest.mark.parametrize("scene", list(SCENES))
@pytest.mark.parametrize("route", ["device_photons", "device_photons_path"])
def test_one_library_call_per_frame_with_the_expected_arguments(scene, route):
    """depth 2, half of the rays have a child, two frames: per frame set_lights, the host-only size query and ONE
    render_recursion_photons straight into d_rgb -- no gen_eye_rays, no per-level call, no gather_level.  The arguments are the
    renderer's sampling, the route's children, capacity fan x samples, the two maps, nphotons and max_dist; workspace and counters
    are the same two tensors in both frames; the per-level list comes from the counters.  No resident rays are needed."""
    path = route == "device_photons_path"
    kw = dict(path_tracing=True, path_kinds=7, path_seed=5) if path else {}
    sc, fr, per_level = render(scene, resident=False, frames=2, depth=2, lights=LIGHTS, fused=route, photon_maps=MAPS, nphotons=50,
                               max_dist=2.0, **kw)
    assert names(sc) == ["set_lights", "recursion_photons_workspace_bytes", "render_recursion_photons"] * 2
    assert per_level == [(N, N * 3 // 4), (N // 2, N // 2 * 3 // 4), (N // 4, N // 4 * 3 // 4)]
    fan = 4 if path else 3
    (_, q, qk), (_, a, k), (_, a2, k2) = sc.calls[1], sc.calls[2], sc.calls[5]
    assert q[1:5] == [W, H, 2, fan * N] and (qk["y0"], qk["y1"], qk["spp"]) == (0, H, SPP)
    assert a[1:3] == [W, H] and a[3][1] == "d_rgb" and a[5] == 2 and a[4][2] == [3, 8] and a[4][3] == "torch.int64"
    assert a[6] == {"type": "FakeMap"} and a[7] == {"type": "FakeMap"} and (k["nphotons"], k["max_dist"]) == (50, 2.0)
    assert (k["y0"], k["y1"], k["spp"], k["jitter"], k["seed"], k["tiled"], k["flags"]) == (0, H, SPP, True, 168, False, 0)
    assert k["children"] == (PATH if path else SPECULAR) and k["environment"] is False
    assert (k["kinds"], k["path_seed"]) == ((7, 5) if path else (3, 168))
    assert k["queue_capacity"] == fan * N and k["workspace_bytes"] == workspace(N, 2, fan * N, path, False)
    assert a[8][2] == [k["workspace_bytes"]] and a[8][3] == "torch.uint8"
    assert (a2[4], a2[8], a2[3]) == (a[4], a[8], a[3])                            # the same three tensors in the second frame
    assert fr.bytes_resident() >= k["workspace_bytes"] + 3 * 8 * 8


def test_one_map_queue_capacity_environment_bands_and_depth_0():
    sc, fr, per_level = render(depth=1, lights=LIGHTS, fused="device_photons", queue_capacity=N, photon_maps=(None, MAPS[1]))
    a, k = sc.calls[2][1], sc.calls[2][2]
    assert a[6] is None and a[7] == {"type": "FakeMap"} and k["queue_capacity"] == N and (k["nphotons"], k["max_dist"]) == (500, 1e10)
    sc, fr, _ = render(depth=1, lights=LIGHTS, fused="device_photons_path", path_tracing=True, path_kinds=7, photon_maps=MAPS,
                       environment=dict(bg_color=(0.1, 0.2, 0.3)))
    assert names(sc) == ["set_environment", "get_environment", "set_lights", "recursion_photons_workspace_bytes", "render_recursion_photons"]
    k = sc.calls[4][2]
    assert k["environment"] is True and k["workspace_bytes"] == workspace(N, 1, 4 * N, True, True)
    sc, fr, per_level = render(bands=[(2, 7)], depth=0, lights=LIGHTS, fused="device_photons", photon_maps=MAPS)
    a, k = sc.calls[2][1], sc.calls[2][2]
    n = 5 * W * SPP
    assert (k["y0"], k["y1"], a[5]) == (2, 7, 0) and k["workspace_bytes"] == 76 * n and a[8][2] == [76 * n]  # a workspace at depth 0 too
    assert per_level == [(n, n * 3 // 4)]
    sc, fr, per_level = render(child=(0, 1), depth=3, lights=LIGHTS, fused="device_photons", photon_maps=MAPS)
    assert len(per_level) == 1 and names(sc).count("render_recursion_photons") == 1     # a queue that dies out: one entry
    sc, fr, per_level = render(bands=[], depth=3, lights=LIGHTS, fused="device_photons", photon_maps=MAPS)
    assert names(sc) == ["set_lights"] and per_level == []
    with pytest.raises(RuntimeError) as e:
        render(depth=2, lights=LIGHTS, fused="device_photons", queue_capacity=100, photon_maps=MAPS)
    assert "level 0" in str(e.value) and str(N // 2) in str(e.value) and "100" in str(e.value), str(e.value)


def test_refusals_name_the_route_that_serves_the_case():
    ok = dict(depth=1, lights=LIGHTS, photon_maps=MAPS)
    path = dict(ok, path_tracing=True)
    cases = [
        ({}, dict(depth=1, lights=LIGHTS, fused="device_photons"), 'fused="device_lights"'),                # no maps
        ({}, dict(depth=1, lights=LIGHTS, path_tracing=True, fused="device_photons_path"), 'fused="device_lights_path"'),
        (dict(tiled=True), dict(ok, fused="device_photons"), 'fused="lights"'),
        (dict(tiled=True), dict(path, fused="device_photons_path"), 'fused="lights_path"'),
        (dict(lens=dict(aperture=0.1, focus_plane=4.0)), dict(ok, fused="device_photons"), "batched"),
        (dict(bands=[(0, 2), (4, 6)]), dict(ok, fused="device_photons"), 'fused="lights"'),
        (dict(bands=[(0, 2), (4, 6)]), dict(path, fused="device_photons_path"), 'fused="lights_path"'),
        (dict(square=True), dict(ok, fused="device_photons"), "batched"),
        ({}, dict(ok, fused="device_photons", group_octants=True), "batched"),
        # the other checks of "frame_lights" / "frame_lights_path"
        ({}, dict(depth=1, photon_maps=MAPS, fused="device_photons"), "lights=[...]"),
        ({}, dict(path, fused="device_photons"), "path_tracing"),
        ({}, dict(ok, fused="device_photons_path"), "path_tracing=True"),
        ({}, dict(ok, fused="device_photons", surface_children=True), "surface_children=True"),
        ({}, dict(path, fused="device_photons_path", surface_children=False), "surface_children=False"),
        # unchanged: the map-less routes send a caller with maps to the per-level driver
        ({}, dict(ok, fused="device_lights"), 'fused="frame_lights"'),
        ({}, dict(path, fused="device_lights_path"), 'fused="frame_lights_path"'),
    ]
    for make, kw, word in cases:
        with pytest.raises(ValueError) as e:
            render(**make, **kw)
        assert word in str(e.value), (word, str(e.value))


def test_no_recorded_case_makes_the_new_call():
    """tests/golden/render_specular_calls.json stays true (tests/test_frame_plan.py checks every case): fused="auto" and every other
    recorded value of `fused` never reach the new routes"""
    with open(GOLDEN) as fh:
        golden = json.load(fh)
    for case in CASES:
        assert "render_recursion_photons" not in golden[case]["calls"], case


def test_gather_queued_kernels_stay_inside_the_verified_envelope():
    """Every kernel of mr_gather_queued.hip: no dynamic stack; the queued estimate without STATS at five waves per SIMD or more and
    at most 4 spilled VGPRs, what tests/test_build_budget.py holds its host-n twin to; no more spilled VGPRs, no more scratch per
    lane and no fewer waves than BOTH its own record (tests/golden/kernel_budget_gather_queued.json, written from the build whose
    GPU run of tests/test_recursion_photons.py was green) AND the worst value among the kernels of tests/golden/kernel_budget.json.
    Five kernels: the two query kernels, the two builds of the estimate, the accumulate."""
    cur = kernel_budget.unit_kernels("mr_gather_queued")
    for needle in ("gather_queued_queries_kernel", "gather_eye_queries_kernel", "irradiance_queued_kernelILb0", "irradiance_queued_kernelILb1",
                   "gather_queued_accumulate_kernel"):
        assert sum(needle in k for k in cur) == 1, needle
    assert len(cur) == 5
    assert not any(v["dynamic_stack"] for v in cur.values())
    (lean,) = [v for k, v in cur.items() if "irradiance_queued_kernelILb0" in k]
    assert lean["waves_per_simd"] >= 5 and lean["vgprs_spilled"] <= 4, lean
    kernel_budget.assert_inside_envelope(cur, "kernel_budget_gather_queued.json", also_main=True)
