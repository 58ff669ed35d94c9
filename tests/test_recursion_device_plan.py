"""mr_render_recursion without a GPU (include/miro_hip_recursion.h, csrc/mr_level_lights_queued.hip): the two symbols and their
list, the descriptor against the header's text, the workspace formula, the argument errors before any device call, what
render_specular(fused="device_lights" | "device_lights_path") hands to the library -- recorded by the stand-in scene of
tests/test_frame_plan.py, extended by the one call this route makes --, what the route refuses, that every other value of `fused`
launches what it launched before, and the unit's kernels against their golden record."""
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
from test_frame_plan import CASES, DESC, GOLDEN, LIGHTS, SCENES, SQUARE, FakeMap, RecordingScene, run_case, summary  # noqa: E402

NAMES = ["mr_render_recursion_workspace", "mr_render_recursion"]
W, H, SPP = 16, 8, 2
N = W * H * SPP
SPECULAR, PATH = binding.MR_LEVEL_SPECULAR, binding.MR_LEVEL_PATH


def header(name):
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", name)).read(), flags=re.S)


def test_the_two_symbols_are_exported_declared_and_bound(miro):
    """Fails on the parent commit: the symbols, the header and the fifth list are this feature's.  The older four lists are as
    they were, and miro_hip.h alone reaches the new header (through miro_hip_render.h, its last include)."""
    for name in NAMES:
        declared = lambda h: re.search(r"\bmr_status\s+%s\s*\(" % name, header(h)) is not None              # noqa: E731
        assert hasattr(miro.lib(), name) and getattr(miro.lib(), name).restype is C.c_int32
        assert declared("miro_hip_recursion.h")
        assert not any(declared(h) for h in ("miro_hip.h", "miro_hip_surface.h", "miro_hip_frame.h", "miro_hip_render.h"))
        assert name not in binding.RENDER_SYMBOLS + binding.FRAME_SYMBOLS + binding.SURFACE_SYMBOLS + miro.EXPORTED_SYMBOLS
    assert binding.RECURSION_SYMBOLS == NAMES
    assert len(miro.EXPORTED_SYMBOLS) == 69 and len(binding.SURFACE_SYMBOLS) == 9 and len(binding.FRAME_SYMBOLS) == 3
    assert binding.RENDER_SYMBOLS == ["mr_render_level_lights"]
    top = open(os.path.join(ROOT, "include", "miro_hip.h")).read()
    assert top.rstrip().endswith('#include "miro_hip_render.h"\n#endif /* MIRO_HIP_H */')
    assert '#include "miro_hip_recursion.h"' in header("miro_hip_render.h")
    assert hasattr(miro.Scene, "render_recursion") and hasattr(miro.Scene, "recursion_workspace_bytes")


def test_recursion_desc_matches_the_header():
    """sizeof and the offsets, worked out from the header's own field list: twelve 32-bit words and nothing else"""
    body = re.search(r"typedef struct mr_recursion_desc \{(.*?)\} mr_recursion_desc;", header("miro_hip_recursion.h"), re.S).group(1)
    fields = [f.strip() for f in body.split(";") if f.strip()]
    names, sizes = [], []
    for f in fields:
        assert f.startswith("uint32_t"), f
        for name in f[len("uint32_t"):].split(","):
            m = re.search(r"\[(\d+)\]", name)
            names.append(re.sub(r"\[\d+\]", "", name).strip())
            sizes.append(int(m.group(1)) if m else 1)
    D = binding.RecursionDesc
    assert [n for n, _ in D._fields_] == names == ["depth", "children", "environment", "path_kinds", "path_seed", "queue_capacity_lo",
                                                   "queue_capacity_hi", "reserved"]
    assert C.sizeof(D) == 4 * sum(sizes) == 48
    off = 0
    for name, words in zip(names, sizes):
        assert getattr(D, name).offset == off and getattr(D, name).size == 4 * words
        off += 4 * words


def workspace(capacity, path, env):
    """the header's formula: two queues; per queue 32 + 12 + 4 bytes per ray, + 4 (id) under MR_LEVEL_PATH, + 1 (low-res byte)
    under MR_LEVEL_PATH with an environment; every array starts on a multiple of 16 bytes"""
    up = lambda v: (v + 15) // 16 * 16                                                                       # noqa: E731
    per_ray = [32, 12, 4] + ([4] if path else []) + ([1] if path and env else [])
    return 2 * sum(up(b * capacity) for b in per_ray)


def rdesc(depth=3, children=SPECULAR, environment=0, kinds=7, capacity=100, reserved=None):
    rd = binding.RecursionDesc()
    rd.depth, rd.children, rd.environment, rd.path_kinds, rd.path_seed = depth, children, environment, kinds, 168
    rd.queue_capacity_lo, rd.queue_capacity_hi = capacity & 0xFFFFFFFF, capacity >> 32
    if reserved is not None:
        rd.reserved[reserved] = 1
    return rd


def test_workspace_bytes_is_the_formula(miro):
    L = miro.lib()
    out = C.c_uint64(12345)
    for capacity in (1, 100, 257, 4099, 3 * 1920 * 1080):
        for children in (SPECULAR, PATH):
            for env in (0, 1):
                assert L.mr_render_recursion_workspace(C.byref(rdesc(3, children, env, capacity=capacity)), C.byref(out)) == binding.MR_OK
                assert out.value == workspace(capacity, children == PATH, env), (capacity, children, env)
                assert out.value >= 2 * capacity * (48 + (4 if children == PATH else 0) + (1 if children == PATH and env else 0))
                assert L.mr_render_recursion_workspace(C.byref(rdesc(0, children, env, capacity=capacity)), C.byref(out)) == binding.MR_OK
                assert out.value == 0
    assert L.mr_render_recursion_workspace(C.byref(rdesc(0, children=0, capacity=0)), C.byref(out)) == binding.MR_OK and out.value == 0
    out.value = 777
    bad = [("NULL", (None, C.byref(out))), ("NULL", (C.byref(rdesc()), None)), ("reserved", (C.byref(rdesc(reserved=0)), C.byref(out))),
           ("reserved", (C.byref(rdesc(reserved=4)), C.byref(out))), ("depth", (C.byref(rdesc(depth=65)), C.byref(out))),
           ("children", (C.byref(rdesc(children=0)), C.byref(out))), ("queue_capacity", (C.byref(rdesc(capacity=0)), C.byref(out))),
           ("path_kinds", (C.byref(rdesc(children=PATH, kinds=0)), C.byref(out))),
           ("environment", (C.byref(rdesc(environment=2)), C.byref(out)))]
    for word, args in bad:
        assert L.mr_render_recursion_workspace(*args) == binding.MR_ERR_INVALID, word
        msg = L.mr_last_error()
        assert word.encode() in msg and b"mr_render_recursion_workspace" in msg, (word, msg)
    assert out.value == 777                                                       # a refused call writes nothing


def test_argument_errors_come_before_the_scene_and_the_device(miro):
    """Every MR_ERR_INVALID case on a host_only one-triangle scene: answered from the arguments alone, under this call's name,
    before any device call, so "no HIP device" and "host_only" may not be what comes back.  mr_render_level_lights' own cases
    first, then this call's.  Then MR_ERR_STATE for that scene, for an unbuilt one and for one without lights."""
    L = miro.lib()
    s = miro.Scene()
    s.add_triangle([0, 0, 0, 1, 0, 0, 0, 1, 0], [0, 0, 1] * 3)
    s.set_lights([dict(position=(0, 1, 0), wattage=5.0)])
    s.build(4, host_only=True)
    p = lambda a: C.c_void_p(a)                                                   # noqa: E731
    need = workspace(100, False, 0)
    base = dict(scene=s.h, rgb=p(8192), ws=p(1 << 20), bytes=need, counts=p(1 << 16))

    def call(fd, rd, **kw):
        a = dict(base, **kw)
        st = L.mr_render_recursion(a["scene"], C.byref(fd) if fd is not None else None, C.byref(rd) if rd is not None else None,
                                   a["rgb"], a["ws"], a["bytes"], a["counts"], None)
        return st, L.mr_last_error()

    fd, ok = frame_desc(binding), rdesc()
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
        ("queue_capacity", call(fd, rdesc(capacity=0))),
        ("workspace", call(fd, ok, ws=None)), ("workspace", call(fd, ok, ws=p((1 << 20) + 8))),
        ("workspace_bytes", call(fd, ok, bytes=need - 1)), ("workspace_bytes", call(fd, ok, bytes=0)),
        ("workspace_bytes", call(fd, rdesc(children=PATH), bytes=need)),
    ]
    for word, (st, msg) in invalid:
        assert st == binding.MR_ERR_INVALID, (word, st, msg)
        assert word.encode() in msg and b"mr_render_recursion" in msg and b"HIP device" not in msg and b"host_only" not in msg, (word, msg)
    for good in (call(fd, ok), call(fd, rdesc(depth=0, children=0, capacity=0), ws=None, bytes=0), call(fd, rdesc(depth=64))):
        st, msg = good                                                            # then the scene's state: never a CPU path
        assert st == binding.MR_ERR_STATE and (b"CPU" in msg or b"device" in msg) and b"HIP device" not in msg, msg
    unbuilt = miro.Scene()
    unbuilt.add_triangle([0, 0, 0, 1, 0, 0, 0, 1, 0], [0, 0, 1] * 3)
    st, msg = call(fd, ok, scene=unbuilt.h)
    assert st == binding.MR_ERR_STATE and b"mr_bvh_build" in msg, msg
    st, msg = call(fd, rdesc(reserved=2), scene=unbuilt.h)
    assert st == binding.MR_ERR_INVALID and b"reserved" in msg                    # still the arguments first
    s.set_lights([])
    st, msg = call(fd, ok)
    assert st == binding.MR_ERR_STATE and b"HIP device" not in msg, msg
    assert s.info().n_triangles == 1                                              # the refused calls left the scene alone


# ---- the driver, recorded -----------------------------------------------------------------------------------------------------
class Recorder(RecordingScene):
    """RecordingScene that answers recursion_workspace_bytes with the header's formula and does to d_level_counts what
    mr_render_recursion would: `hit` of a level's rays cast a shadow ray, `child` of them have a child, a queue holds `capacity`"""

    def launch(self, name, a, kw):
        if name == "recursion_workspace_bytes":
            return 0 if a[0] == 0 else workspace(a[1], kw["children"] == PATH, kw["environment"])
        if name != "render_recursion":
            assert name not in ("render_level_lights", "trace_level_lights", "trace_level_lights_path"), name
            return super().launch(name, a, kw)
        counts, depth = a[4], a[5]
        n = (kw["y1"] - kw["y0"]) * a[1] * kw["spp"]
        counts.zero_()
        for level in range(depth + 1):
            counts[level, 0], counts[level, 1] = n, self.part(n, self.hit)
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


@pytest.mark.parametrize("scene", list(SCENES))
@pytest.mark.parametrize("route", ["device_lights", "device_lights_path"])
def test_one_library_call_per_frame_with_the_expected_descriptor(scene, route):
    """depth 2, half of the rays have a child, two frames: per frame set_lights, the host-only size query and ONE render_recursion
    straight into d_rgb -- no gen_eye_rays, no per-level call, no untile_pixels.  The descriptor is the renderer's sampling, the
    route's children, capacity fan x samples; workspace and counters are the same two tensors in both frames; the per-level list
    comes from the counters.  A renderer without resident rays serves."""
    path = route == "device_lights_path"
    kw = dict(path_tracing=True, path_kinds=7, path_seed=5) if path else {}
    sc, fr, per_level = render(scene, resident=False, frames=2, depth=2, lights=LIGHTS, fused=route, **kw)
    assert names(sc) == ["set_lights", "recursion_workspace_bytes", "render_recursion"] * 2
    assert per_level == [(N, N * 3 // 4), (N // 2, N // 2 * 3 // 4), (N // 4, N // 4 * 3 // 4)]
    fan = 4 if path else 3
    (_, a, k), (_, a2, k2) = sc.calls[2], sc.calls[5]
    assert a[1:3] == [W, H] and a[3][1] == "d_rgb" and a[5] == 2 and a[4][2] == [3, 8] and a[4][3] == "torch.int64"
    assert (k["y0"], k["y1"], k["spp"], k["jitter"], k["seed"], k["tiled"], k["flags"]) == (0, H, SPP, True, 168, False, 0)
    assert k["children"] == (PATH if path else SPECULAR) and k["environment"] is False
    assert (k["kinds"], k["path_seed"]) == ((7, 5) if path else (3, 168))
    assert k["queue_capacity"] == fan * N and k["workspace_bytes"] == workspace(fan * N, path, False)
    assert k["d_workspace"][2] == [k["workspace_bytes"]] and k["d_workspace"][3] == "torch.uint8"
    assert (a2[4], k2["d_workspace"], a2[3]) == (a[4], k["d_workspace"], a[3])    # the same three tensors in the second frame
    assert fr.bytes_resident() >= k["workspace_bytes"] + 3 * 8 * 8


def test_queue_capacity_environment_tiled_and_depth_0():
    sc, fr, per_level = render("table", tiled=True, depth=1, lights=LIGHTS, fused="device_lights", queue_capacity=N)
    k = sc.calls[2][2]
    assert names(sc) == ["set_lights", "recursion_workspace_bytes", "render_recursion"] and k["tiled"] is True and fr.tiled
    assert k["queue_capacity"] == N and sc.calls[2][1][3][1] == "d_rgb" and fr.d_slots.data_ptr() != fr.d_rgb.data_ptr()
    sc, fr, _ = render(depth=1, lights=LIGHTS, fused="device_lights_path", path_tracing=True, path_kinds=7,
                       environment=dict(bg_color=(0.1, 0.2, 0.3)))
    assert names(sc) == ["set_environment", "get_environment", "set_lights", "recursion_workspace_bytes", "render_recursion"]
    k = sc.calls[4][2]
    assert k["environment"] is True and k["workspace_bytes"] == workspace(4 * N, True, True)
    sc, fr, per_level = render(bands=[(2, 7)], depth=0, lights=LIGHTS, fused="device_lights")
    k = sc.calls[2][2]
    assert (k["y0"], k["y1"], k["d_workspace"], k["workspace_bytes"]) == (2, 7, None, 0) and sc.calls[2][1][5] == 0
    assert per_level == [(5 * W * SPP, 5 * W * SPP * 3 // 4)]
    sc, fr, per_level = render(child=(0, 1), depth=3, lights=LIGHTS, fused="device_lights")
    assert len(per_level) == 1 and names(sc).count("render_recursion") == 1       # a queue that dies out: one entry
    sc, fr, per_level = render(bands=[], depth=3, lights=LIGHTS, fused="device_lights")
    assert names(sc) == ["set_lights"] and per_level == []


def test_a_truncated_level_raises_with_the_level_and_the_two_numbers():
    with pytest.raises(RuntimeError) as e:
        render(depth=2, lights=LIGHTS, fused="device_lights", queue_capacity=100)
    assert "level 0" in str(e.value) and str(N // 2) in str(e.value) and "100" in str(e.value), str(e.value)
    sc, fr, per_level = render(depth=2, lights=LIGHTS, fused="device_lights", queue_capacity=N // 2)   # exactly full is not truncated
    assert len(per_level) == 3


def test_refusals_name_the_route_that_serves_the_case():
    ok = dict(depth=1, lights=LIGHTS)
    path = dict(ok, path_tracing=True)
    cases = [
        (dict(lens=dict(aperture=0.1, focus_plane=4.0)), dict(ok, fused="device_lights"), "batched"),
        (dict(bands=[(0, 2), (4, 6)]), dict(ok, fused="device_lights"), 'fused="lights"'),
        (dict(bands=[(0, 2), (4, 6)]), dict(path, fused="device_lights_path"), 'fused="lights_path"'),
        ({}, dict(ok, fused="device_lights", photon_maps=(FakeMap(), None)), 'fused="frame_lights"'),
        ({}, dict(path, fused="device_lights_path", photon_maps=(FakeMap(), None)), 'fused="frame_lights_path"'),
        (dict(square=True), dict(ok, fused="device_lights"), "square lights"),
        ({}, dict(ok, fused="device_lights", group_octants=True), "group_octants"),
        # the other checks of "frame_lights" / "frame_lights_path"
        ({}, dict(depth=1, fused="device_lights"), "lights=[...]"),
        ({}, dict(path, fused="device_lights"), "path_tracing"),
        ({}, dict(ok, fused="device_lights_path"), "path_tracing=True"),
        ({}, dict(ok, fused="device_lights", surface_children=True), "surface_children=True"),
        ({}, dict(path, fused="device_lights_path", surface_children=False), "surface_children=False"),
    ]
    for make, kw, word in cases:
        with pytest.raises(ValueError) as e:
            render(**make, **kw)
        assert word in str(e.value), (word, str(e.value))
    with pytest.raises(ValueError) as e:                                          # square lights and group_octants: the batched path
        render(square=True, **dict(ok, fused="device_lights"))
    assert "batched" in str(e.value)
    with pytest.raises(ValueError) as e:
        render(**dict(ok, fused="device_lights", group_octants=True))
    assert "batched" in str(e.value)


def test_every_other_value_of_fused_launches_what_it_launched_before():
    """the recorded sequences of tests/golden/render_specular_calls.json hold (tests/test_frame_plan.py checks every case; here one
    of each value of `fused`), no case of them makes the new call -- fused="auto" never picks it -- and the frame routes still make
    their launch per level"""
    with open(GOLDEN) as fh:
        golden = json.load(fh)
    for case in CASES:
        assert "render_recursion" not in golden[case]["calls"], case
    for case in ("plain-nosquare-auto_half_hit", "plain-nosquare-auto_all_hit", "table-nosquare-fused", "procedural-square-path7",
                 "table-nosquare-lights", "plain-nosquare-photon_lights", "procedural-nosquare-depth2"):
        got = run_case(case)
        assert summary(got) == golden[case], case
        assert "render_recursion" not in [c[0] for c in got["calls"]]
    from test_frame_level_lights_plan import render as frame_render
    sc, fr, _ = frame_render("table", depth=2, lights=LIGHTS, fused="frame_lights")
    assert [c[0] for c in sc.calls] == ["set_lights", "render_level_lights", "trace_level_lights", "trace_level_lights"]
    sc, fr, _ = frame_render("table", tiled=True, depth=1, lights=LIGHTS, fused="lights")
    assert [c[0] for c in sc.calls] == ["set_lights", "trace_level_lights", "trace_level_lights", "untile_pixels"]


def test_queued_level_kernels_stay_inside_the_verified_envelope():
    """Every kernel of mr_level_lights_queued.hip: no dynamic stack; at least four waves per SIMD; no more spilled VGPRs, no more
    scratch per lane and no fewer waves than BOTH its own record (tests/golden/kernel_budget_level_lights_queued.json, written
    from the build whose GPU run of tests/test_recursion_device.py was green) AND the worst value among the kernels of
    tests/golden/kernel_budget.json.  One level kernel per traversal variant of with_trace_variant (six), CHILDREN 0 / 1 and build
    (specular, path tracing), and the kernel that zeroes the counters."""
    cur = kernel_budget.unit_kernels("mr_level_lights_queued")
    variants, children, builds = (1818, 826, 267, 43, 88, 73), (0, 1), ("level_lights_queued_kernel", "level_lights_path_queued_kernel")
    level = [k for k in cur if "queued_kernel" in k]
    assert len(level) == len(variants) * len(children) * len(builds)
    for build in builds:
        for var in variants:
            for ch in children:
                assert sum("%sILi%dELi%dEE" % (build, var, ch) in k for k in cur) == 1, (build, var, ch)
    other = sorted(set(cur) - set(level))
    assert len(other) == 1 and "zero_words_kernel" in other[0]
    assert not any(v["dynamic_stack"] for v in cur.values())
    assert all(v["waves_per_simd"] >= 4 for v in cur.values())
    kernel_budget.assert_inside_envelope(cur, "kernel_budget_level_lights_queued.json", also_main=True)
