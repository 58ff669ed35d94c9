"""The thin-lens forms of the fused frame and of the one-call recursions without a GPU (include/miro_hip_lens.h,
csrc/mr_frame_lens.hip): the three symbols and their list, the argument errors before any device call, what
render_specular(fused="frame_lens[_path]" | "device_lens[_path]" | "device_lens_photons[_path]") hands to the library -- recorded
by the stand-in scene of tests/test_frame_plan.py, extended by the calls these routes make --, what the routes refuse, and the
unit's kernels against their golden record.  That the pinhole routes go on refusing a lens is asserted in their own files."""
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
from test_frame_level_lights import level_desc  # noqa: E402
from test_frame_lights import frame_desc  # noqa: E402
from test_frame_plan import DESC, LIGHTS, SCENES, SQUARE, FakeMap, RecordingScene  # noqa: E402
from test_recursion_device_plan import rdesc, workspace as queues  # noqa: E402
from test_recursion_photons_plan import workspace as photons_workspace  # noqa: E402

NAMES = ["mr_render_level_lights_lens", "mr_render_recursion_lens", "mr_render_recursion_photons_lens"]
HEADERS = ("miro_hip.h", "miro_hip_surface.h", "miro_hip_frame.h", "miro_hip_render.h", "miro_hip_recursion.h",
           "miro_hip_recursion_photons.h")
W, H, SPP = 16, 8, 2
N = W * H * SPP
SPECULAR, PATH = binding.MR_LEVEL_SPECULAR, binding.MR_LEVEL_PATH
LENS = dict(aperture=0.2, focus_plane=6.1)


def header(name):
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", name)).read(), flags=re.S)


def test_the_three_symbols_are_exported_declared_and_bound(miro):
    """Fails on the parent commit: the symbols, the header and the seventh list are this feature's.  The six older lists are as
    they were, and miro_hip.h alone reaches the new header (miro_hip_recursion_photons.h's last line, below its declarations)."""
    for name in NAMES:
        declared = lambda h: re.search(r"\bmr_status\s+%s\s*\(" % name, header(h)) is not None              # noqa: E731
        assert hasattr(miro.lib(), name) and getattr(miro.lib(), name).restype is C.c_int32
        assert declared("miro_hip_lens.h") and not any(declared(h) for h in HEADERS)
        assert name not in (binding.RECURSION_PHOTONS_SYMBOLS + binding.RECURSION_SYMBOLS + binding.RENDER_SYMBOLS + binding.FRAME_SYMBOLS +
                            binding.SURFACE_SYMBOLS + miro.EXPORTED_SYMBOLS)
        assert "Camera.cpp:135-160" in open(os.path.join(ROOT, "include", "miro_hip_lens.h")).read()
    assert binding.LENS_SYMBOLS == NAMES
    assert binding.RECURSION_PHOTONS_SYMBOLS == ["mr_render_recursion_photons_workspace", "mr_render_recursion_photons"]
    assert binding.RECURSION_SYMBOLS == ["mr_render_recursion_workspace", "mr_render_recursion"]
    assert binding.RENDER_SYMBOLS == ["mr_render_level_lights"]
    assert binding.FRAME_SYMBOLS == ["mr_render_lights_environment", "mr_trace_level_lights", "mr_trace_level_lights_path"]
    assert len(miro.EXPORTED_SYMBOLS) == 69 and len(binding.SURFACE_SYMBOLS) == 9 and "mr_gen_eye_rays_lens" in miro.EXPORTED_SYMBOLS
    raw = lambda h: open(os.path.join(ROOT, "include", h)).read().rstrip()                                  # noqa: E731
    assert raw("miro_hip.h").endswith('#include "miro_hip_render.h"\n#endif /* MIRO_HIP_H */')
    assert '#include "miro_hip_recursion.h"' in header("miro_hip_render.h")
    assert raw("miro_hip_recursion.h").endswith('#endif /* MIRO_HIP_RECURSION_H */\n#include "miro_hip_recursion_photons.h"')
    assert raw("miro_hip_recursion_photons.h").endswith('#endif /* MIRO_HIP_RECURSION_PHOTONS_H */\n#include "miro_hip_lens.h"')
    assert raw("miro_hip_lens.h").endswith("#endif /* MIRO_HIP_LENS_H */")
    for method in ("render_level_lights_lens", "render_recursion_lens", "render_recursion_photons_lens"):
        assert hasattr(miro.Scene, method)


def lens_desc(aperture=0.2, focus_plane=6.0, reserved=None):
    ln = binding.LensDesc()
    ln.aperture, ln.focus_plane = aperture, focus_plane
    if reserved is not None:
        ln.reserved[reserved] = 1
    return ln


def tiled_desc():
    fd = frame_desc(binding)
    fd.tiled = 1
    return fd


NAN, INF = float("nan"), float("inf")
LENS_CASES = [("NULL lens", None)] + [("reserved", lens_desc(reserved=k)) for k in range(6)] + \
    [("aperture", lens_desc(aperture=a)) for a in (-0.1, NAN, INF)] + \
    [("focus_plane", lens_desc(focus_plane=f)) for f in (0.0, -1.0, NAN, INF)]


def check_lens_errors(call, name):
    """the lens cases and `tiled` are MR_ERR_INVALID under the call's own name, before the scene's state; aperture 0 passes them"""
    for word, ln in LENS_CASES:
        st, msg = call(frame_desc(binding), ln)
        assert st == binding.MR_ERR_INVALID, (name, word, st, msg)
        assert word.encode() in msg and name.encode() in msg and b"HIP device" not in msg and b"host_only" not in msg, (word, msg)
    st, msg = call(tiled_desc(), lens_desc())
    assert st == binding.MR_ERR_INVALID and b"tiled" in msg and name.encode() in msg and b"host_only" not in msg, msg
    st, msg = call(frame_desc(binding, spp=3), None)                               # the pinhole call's list comes first
    assert st == binding.MR_ERR_INVALID and b"spp" in msg and name.encode() in msg, msg
    for ln in (lens_desc(), lens_desc(aperture=0.0)):                              # then the scene's state: never a CPU path
        st, msg = call(frame_desc(binding), ln)
        assert st == binding.MR_ERR_STATE and (b"CPU" in msg or b"device" in msg) and b"HIP device" not in msg, msg


def host_only_scene(miro):
    s = miro.Scene()
    s.add_triangle([0, 0, 0, 1, 0, 0, 0, 1, 0], [0, 0, 1] * 3)
    s.set_lights([dict(position=(0, 1, 0), wattage=5.0)])
    s.build(4, host_only=True)
    return s


def test_level_lights_lens_argument_errors_come_before_the_scene_and_the_device(miro):
    """mr_render_level_lights' cases under this call's name, then the lens cases, then `tiled`; all three kinds of children are
    served as far as the state check"""
    L = miro.lib()
    s = host_only_scene(miro)
    p = lambda a: C.c_void_p(a)                                                   # noqa: E731
    name = NAMES[0]
    queue = dict(out_rays=p(1 << 16), out_weights=p(1 << 17), out_pixels=p(1 << 18), out_count=p(1 << 19))
    base = dict(scene=s.h, rgb=p(8192), out_rays=None, out_weights=None, out_pixels=None, out_count=None)

    def call(fd, ln, ld=None, **kw):
        a = dict(base, **kw)
        ld = level_desc(binding) if ld is None else ld
        st = getattr(L, name)(a["scene"], C.byref(fd) if fd is not None else None, C.byref(ln) if ln is not None else None,
                              C.byref(ld) if ld != "null" else None, a["rgb"], None, None, None, None, a["out_rays"], a["out_weights"],
                              a["out_pixels"], None, a["out_count"], None, None)
        return st, L.mr_last_error()

    fd, ok = frame_desc(binding), lens_desc()
    spec = level_desc(binding, children=SPECULAR, capacity=256)
    path = level_desc(binding, children=PATH, capacity=256)
    invalid = [
        ("NULL", call(fd, ok, scene=None)), ("NULL", call(None, ok)), ("NULL", call(fd, ok, rgb=None)),
        ("empty image", call(frame_desc(binding, W=0), ok)), ("spp", call(frame_desc(binding, spp=128), ok)),
        ("band", call(frame_desc(binding, bands=(0, 0, 2)), ok)), ("rows", call(frame_desc(binding, y0=5, y1=3), ok)),
        ("aligned", call(fd, ok, rgb=p(8194))),
        ("NULL", call(fd, ok, ld="null")),
        ("flags", call(frame_desc(binding, flags=binding.MR_TRACE_ANY), ok)),
        ("children", call(fd, ok, level_desc(binding, children=7, capacity=256), **queue)),
        ("environment", call(fd, ok, level_desc(binding, environment=2))),
        ("path_kinds", call(fd, ok, level_desc(binding, children=PATH, capacity=256, kinds=0), **queue)),
        ("reserved", call(fd, ok, level_desc(binding, reserved=0))),
        ("output queue", call(fd, ok, spec)), ("out_capacity", call(fd, ok, level_desc(binding, children=PATH), **queue)),
        ("aligned", call(fd, ok, spec, **dict(queue, out_rays=p((1 << 16) + 4)))),
    ]
    for word, (st, msg) in invalid:
        assert st == binding.MR_ERR_INVALID, (word, st, msg)
        assert word.encode() in msg and name.encode() in msg and b"HIP device" not in msg and b"host_only" not in msg, (word, msg)
    st, msg = call(fd, None, level_desc(binding, children=7))                      # a level error comes before a lens error
    assert st == binding.MR_ERR_INVALID and b"children" in msg
    check_lens_errors(call, name)
    for ld, kw in ((spec, queue), (path, queue)):
        st, msg = call(frame_desc(binding, bands=(3, 1, 2)), lens_desc(aperture=0.0), ld, **kw)          # bands are allowed
        assert st == binding.MR_ERR_STATE and b"HIP device" not in msg, msg
    assert s.info().n_triangles == 1


def test_recursion_lens_argument_errors_come_before_the_scene_and_the_device(miro):
    L = miro.lib()
    s = host_only_scene(miro)
    p = lambda a: C.c_void_p(a)                                                   # noqa: E731
    name = NAMES[1]
    need = queues(100, False, 0)
    base = dict(scene=s.h, rgb=p(8192), ws=p(1 << 20), bytes=need, counts=p(1 << 16), rd=rdesc())

    def call(fd, ln, **kw):
        a = dict(base, **kw)
        st = getattr(L, name)(a["scene"], C.byref(fd) if fd is not None else None, C.byref(ln) if ln is not None else None,
                              C.byref(a["rd"]) if a["rd"] is not None else None, a["rgb"], a["ws"], a["bytes"], a["counts"], None)
        return st, L.mr_last_error()

    fd, ok = frame_desc(binding), lens_desc()
    invalid = [
        ("NULL", call(fd, ok, scene=None)), ("NULL", call(None, ok)), ("NULL", call(fd, ok, rgb=None)),
        ("spp", call(frame_desc(binding, spp=3), ok)), ("flags", call(frame_desc(binding, flags=binding.MR_TRACE_ANY), ok)),
        ("aligned", call(fd, ok, counts=p((1 << 16) + 4))), ("NULL", call(fd, ok, rd=None)), ("d_level_counts", call(fd, ok, counts=None)),
        ("depth", call(fd, ok, rd=rdesc(depth=65))), ("children", call(fd, ok, rd=rdesc(children=0))),
        ("path_kinds", call(fd, ok, rd=rdesc(children=PATH, kinds=8))), ("reserved", call(fd, ok, rd=rdesc(reserved=4))),
        ("queue_capacity", call(fd, ok, rd=rdesc(capacity=0))),
        ("workspace", call(fd, ok, ws=None)), ("workspace_bytes", call(fd, ok, bytes=need - 1)),
    ]
    for word, (st, msg) in invalid:
        assert st == binding.MR_ERR_INVALID, (word, st, msg)
        assert word.encode() in msg and name.encode() in msg and b"HIP device" not in msg and b"host_only" not in msg, (word, msg)
    st, msg = call(fd, None, bytes=0)                                              # the workspace comes before the lens
    assert st == binding.MR_ERR_INVALID and b"workspace_bytes" in msg
    check_lens_errors(call, name)
    st, msg = call(fd, lens_desc(aperture=0.0), rd=rdesc(depth=0, children=0, capacity=0), ws=None, bytes=0)
    assert st == binding.MR_ERR_STATE and b"HIP device" not in msg, msg           # depth 0 needs no workspace
    assert s.info().n_triangles == 1


def test_recursion_photons_lens_argument_errors_come_before_the_scene_and_the_device(miro):
    L = miro.lib()
    s = host_only_scene(miro)
    g, c = miro.PhotonMap(64), miro.PhotonMap(64)
    p = lambda a: C.c_void_p(a)                                                   # noqa: E731
    name = NAMES[2]
    fd, ok = frame_desc(binding), lens_desc()
    need = photons_workspace(fd.W * (fd.y1 - fd.y0) * fd.spp, 3, 100, False, 0)
    base = dict(scene=s.h, g=g.h, c=c.h, dist=1e10, k=50, rgb=p(8192), ws=p(1 << 20), bytes=need, counts=p(1 << 16), rd=rdesc())

    def call(fd, ln, **kw):
        a = dict(base, **kw)
        st = getattr(L, name)(a["scene"], C.byref(fd) if fd is not None else None, C.byref(ln) if ln is not None else None,
                              C.byref(a["rd"]) if a["rd"] is not None else None, a["g"], a["c"], a["dist"], a["k"], a["rgb"], a["ws"],
                              a["bytes"], a["counts"], None)
        return st, L.mr_last_error()

    invalid = [
        ("NULL", call(fd, ok, scene=None)), ("NULL", call(None, ok)), ("NULL", call(fd, ok, rgb=None)),
        ("spp", call(frame_desc(binding, spp=3), ok)), ("flags", call(frame_desc(binding, flags=binding.MR_TRACE_ANY), ok)),
        ("NULL", call(fd, ok, rd=None)), ("d_level_counts", call(fd, ok, counts=None)),
        ("depth", call(fd, ok, rd=rdesc(depth=65))), ("reserved", call(fd, ok, rd=rdesc(reserved=0))),
        ("queue_capacity", call(fd, ok, rd=rdesc(capacity=1 << 31))),
        ("both NULL", call(fd, ok, g=None, c=None)), ("nphotons", call(fd, ok, k=513)), ("max_dist", call(fd, ok, dist=NAN)),
        ("workspace", call(fd, ok, ws=None)), ("workspace_bytes", call(fd, ok, bytes=need - 1)),
        ("tiled", call(tiled_desc(), ok)),
    ]
    for word, (st, msg) in invalid:
        assert st == binding.MR_ERR_INVALID, (word, st, msg)
        assert word.encode() in msg and name.encode() in msg, (word, msg)
        assert b"HIP device" not in msg and b"host_only" not in msg and b"balanced" not in msg, (word, msg)
    st, msg = call(fd, None, k=0)                                                  # the photon arguments come before the lens
    assert st == binding.MR_ERR_INVALID and b"nphotons" in msg
    check_lens_errors(call, name)
    assert s.info().n_triangles == 1 and g.count() == 0


# ---- the driver, recorded -----------------------------------------------------------------------------------------------------
class Recorder(RecordingScene):
    """RecordingScene that does to the counters what the three lens calls and the level calls would, and answers the two size
    queries with the headers' formulas"""

    def launch(self, name, a, kw):
        if name == "recursion_workspace_bytes":
            return 0 if a[0] == 0 else queues(a[1], kw["children"] == PATH, kw["environment"])
        if name == "recursion_photons_workspace_bytes":
            return photons_workspace((kw["y1"] - kw["y0"]) * a[1] * kw["spp"], a[3], a[4], kw["children"] == PATH, kw["environment"])
        if name in ("render_recursion_lens", "render_recursion_photons_lens"):
            counts, depth = a[4], a[5]
            n = (kw["y1"] - kw["y0"]) * a[1] * kw["spp"]
            counts.zero_()
            for level in range(depth + 1):
                counts[level, 0], counts[level, 1] = n, self.part(n, self.hit)
                if level < depth:
                    counts[level, 5] = self.part(n, self.child)
                n = min(int(counts[level, 5]), kw["queue_capacity"])
            return None
        if name == "render_level_lights_lens":
            n = (kw["y1"] - kw["y0"]) * a[1] * kw["spp"]
        elif name == "trace_level_lights":
            n = a[3]
        elif name == "trace_level_lights_path":
            n = a[4]
        else:
            assert name not in ("render_level_lights", "render_recursion", "render_recursion_photons", "gen_eye_rays"), name
            return super().launch(name, a, kw)
        kw["d_counts"][0] += n
        kw["d_counts"][1] += self.part(n, self.hit)
        if kw["d_out_count"] is not None:
            kw["d_out_count"][0] = self.part(n, self.child)
        return None


def render(scene="plain", tiled=None, bands=None, lens=LENS, square=False, resident=True, child=(1, 2), **kw):
    sc = Recorder(*SCENES[scene], hit=(3, 4), child=child, image=False)
    fr = frame.FrameRenderer(sc, DESC, W, H, spp=SPP, bands=bands, device=torch.device("cpu"), tiled=tiled, lens=lens,
                             square_lights=SQUARE if square else None, resident_rays=resident)
    for name, t in sorted(vars(fr).items()):                    # the renderer's own buffers go by name
        if isinstance(t, torch.Tensor):
            sc.register(t, name)
    return sc, fr, fr.render_specular(**kw)


def names(sc):
    return [c[0] for c in sc.calls]


MAPS = (FakeMap(), FakeMap())


@pytest.mark.parametrize("scene", list(SCENES))
@pytest.mark.parametrize("route", ["frame_lens", "frame_lens_path"])
def test_frame_lens_is_one_lens_frame_and_the_level_calls(scene, route):
    """depth 2, half of the rays have a child: set_lights, ONE render_level_lights_lens with the renderer's lens straight into
    d_rgb -- no gen_eye_rays*, on a renderer without resident rays -- then the level calls on its children"""
    path = route.endswith("_path")
    kw = dict(path_tracing=True, path_kinds=7, path_seed=5) if path else {}
    sc, fr, per_level = render(scene, resident=False, depth=2, lights=LIGHTS, fused=route, **kw)
    level = "trace_level_lights_path" if path else "trace_level_lights"
    assert names(sc) == ["set_lights", "render_level_lights_lens", level, level]
    assert per_level == [(N, N * 3 // 4), (N // 2, N // 2 * 3 // 4), (N // 4, N // 4 * 3 // 4)]
    _, a, k = sc.calls[1]
    assert a[1:3] == [W, H] and a[3][1] == "d_rgb" and a[4:] == [LENS["aperture"], LENS["focus_plane"]]
    assert (k["y0"], k["y1"], k["spp"], k["jitter"], k["seed"], k["tiled"]) == (0, H, SPP, True, 168, False)
    assert k["children"] == (PATH if path else SPECULAR) and (k["kinds"], k["path_seed"]) == ((7, 5) if path else (3, 168))
    assert sc.calls[2][1][5 if path else 4][1] == "d_rgb"                          # the further levels add into d_rgb


def test_frame_lens_with_maps_generates_lens_rays():
    sc, fr, per_level = render(depth=1, lights=LIGHTS, fused="frame_lens", photon_maps=MAPS, nphotons=50, max_dist=2.0)
    assert names(sc) == ["set_lights", "gen_eye_rays_lens", "render_level_lights_lens", "gather_level", "trace_level_lights", "gather_level"]
    gen = sc.calls[1][1]
    assert gen[4:6] == [LENS["aperture"], LENS["focus_plane"]]
    sc, fr, per_level = render(bands=[(2, 7)], depth=0, lights=LIGHTS, fused="frame_lens")
    assert names(sc) == ["set_lights", "render_level_lights_lens"] and (sc.calls[1][2]["y0"], sc.calls[1][2]["y1"]) == (2, 7)
    assert sc.calls[1][2]["children"] == binding.MR_LEVEL_LAST and per_level == [(5 * W * SPP, 5 * W * SPP * 3 // 4)]


@pytest.mark.parametrize("route", ["device_lens", "device_lens_path", "device_lens_photons", "device_lens_photons_path"])
def test_device_lens_is_one_library_call(route):
    """per frame set_lights, the host-only size query and ONE render_recursion[_photons]_lens with the renderer's lens; no
    gen_eye_rays*, no per-level call"""
    path, photons = route.endswith("_path"), "photons" in route
    kw = dict(path_tracing=True, path_kinds=7, path_seed=5) if path else {}
    if photons:
        kw.update(photon_maps=MAPS, nphotons=50, max_dist=2.0)
    sc, fr, per_level = render(resident=False, depth=2, lights=LIGHTS, fused=route, **kw)
    call = "render_recursion_photons_lens" if photons else "render_recursion_lens"
    assert names(sc) == ["set_lights", "recursion_photons_workspace_bytes" if photons else "recursion_workspace_bytes", call]
    assert per_level == [(N, N * 3 // 4), (N // 2, N // 2 * 3 // 4), (N // 4, N // 4 * 3 // 4)]
    _, a, k = sc.calls[2]
    fan = 4 if path else 3
    assert a[1:3] == [W, H] and a[3][1] == "d_rgb" and a[5] == 2 and a[4][2] == [3, 8]
    assert (k["aperture"], k["focus_plane"]) == (LENS["aperture"], LENS["focus_plane"])
    assert (k["y0"], k["y1"], k["spp"], k["jitter"], k["seed"], k["tiled"], k["flags"]) == (0, H, SPP, True, 168, False, 0)
    assert k["children"] == (PATH if path else SPECULAR) and k["queue_capacity"] == fan * N
    if photons:
        assert a[6] == {"type": "FakeMap"} and a[7] == {"type": "FakeMap"} and (k["nphotons"], k["max_dist"]) == (50, 2.0)
        assert k["workspace_bytes"] == photons_workspace(N, 2, fan * N, path, False)
    else:
        assert k["workspace_bytes"] == queues(fan * N, path, False)


def test_refusals_name_the_route_that_serves_the_case():
    ok = dict(depth=1, lights=LIGHTS)
    path = dict(ok, path_tracing=True)
    maps = dict(ok, photon_maps=MAPS)
    cases = [
        # without a lens: the pinhole route
        (dict(lens=None), dict(ok, fused="frame_lens"), 'fused="frame_lights"'),
        (dict(lens=None), dict(path, fused="frame_lens_path"), 'fused="frame_lights_path"'),
        (dict(lens=None), dict(ok, fused="device_lens"), 'fused="device_lights"'),
        (dict(lens=None), dict(path, fused="device_lens_path"), 'fused="device_lights_path"'),
        (dict(lens=None), dict(maps, fused="device_lens_photons"), 'fused="device_photons"'),
        (dict(lens=None), dict(maps, path_tracing=True, fused="device_lens_photons_path"), 'fused="device_photons_path"'),
        (dict(lens=None), dict(ok, fused="frame_lens"), "lens=dict("),
        # the checks of the pinhole twin, under this route's name
        ({}, dict(ok, fused="device_lens_photons"), 'fused="device_lens"'),                                # no maps
        ({}, dict(maps, fused="device_lens"), 'fused="frame_lens"'),                                      # maps on the map-less call
        (dict(bands=[(0, 2), (4, 6)]), dict(ok, fused="frame_lens"), 'fused="lights"'),
        (dict(bands=[(0, 2), (4, 6)]), dict(path, fused="device_lens_path"), 'fused="lights_path"'),
        (dict(square=True), dict(ok, fused="frame_lens"), "batched"),
        ({}, dict(ok, fused="device_lens", group_octants=True), "batched"),
        ({}, dict(depth=1, fused="frame_lens"), "lights=[...]"),
        ({}, dict(path, fused="frame_lens"), "path_tracing"),
        ({}, dict(ok, fused="device_lens_path"), "path_tracing=True"),
        ({}, dict(ok, fused="frame_lens", surface_children=True), "surface_children=True"),
        (dict(resident=False), dict(maps, fused="frame_lens"), "resident_rays"),
    ]
    for make, kw, word in cases:
        with pytest.raises(ValueError) as e:
            render(**make, **kw)
        assert word in str(e.value), (word, str(e.value))
    with pytest.raises(ValueError, match="image order"):                           # the constructor refuses tiled with a lens
        render(tiled=True, **dict(ok, fused="frame_lens"))


def test_frame_lens_kernels_stay_inside_the_verified_envelope():
    """Every kernel of mr_frame_lens.hip: the record knows exactly the nineteen -- eighteen frame kernels, one per traversal
    variant of with_trace_variant (six) and CHILDREN 0, 1, 2, and the lens form of the level-0 query kernel --; no dynamic stack;
    at least four waves per SIMD; no more spilled VGPRs, no more scratch per lane and no fewer waves than BOTH its own record
    (tests/golden/kernel_budget_frame_lens.json) AND the worst value among the kernels of tests/golden/kernel_budget.json."""
    cur = kernel_budget.unit_kernels("mr_frame_lens")
    frame_kernels = [k for k in cur if "frame_lens_kernel" in k]
    assert len(frame_kernels) == 6 * 3 and len(cur) == 19
    assert sum("gather_eye_queries_lens_kernel" in k for k in cur) == 1
    for var in (1818, 826, 267, 43, 88, 73):                   # kTraceExact, ExactObj, Product, ProductObj, Vote, VoteProduct
        for children in (0, 1, 2):
            assert sum("ILi%dELi%dEE" % (var, children) in k for k in cur) == 1, (var, children)
    rec = json.load(open(os.path.join(ROOT, "tests", "golden", "kernel_budget_frame_lens.json")))["kernels"]
    assert sorted(rec) == sorted(cur)
    assert not any(v["dynamic_stack"] for v in cur.values())
    assert all(v["waves_per_simd"] >= 4 for v in cur.values())
    kernel_budget.assert_inside_envelope(cur, "kernel_budget_frame_lens.json", also_main=True)
