"""The sample passes and the image finish without a GPU (include/miro_hip_passes.h, csrc/mr_frame_passes.hip): the four symbols and
their list, mr_passes_desc against the header's text, the plan mr_render_passes_plan states, every refusal of
mr_render_recursion_passes / mr_render_recursion_photons_passes / mr_finish_image by its message and before any device call (the
way tests/test_recursion_device_plan.py does it: on a host_only scene, where "no HIP device" may not be what comes back), and what
render_specular(samples=...) refuses."""
import ctypes as C
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kernel_budget  # noqa: E402
from miro_amd import binding  # noqa: E402
from test_frame_lens_plan import lens_desc  # noqa: E402
from test_frame_lights import frame_desc  # noqa: E402
from test_recursion_device_plan import rdesc, workspace  # noqa: E402

NAMES = ["mr_render_passes_plan", "mr_render_recursion_passes", "mr_render_recursion_photons_passes", "mr_finish_image"]
OLDER = ("miro_hip.h", "miro_hip_surface.h", "miro_hip_frame.h", "miro_hip_render.h", "miro_hip_recursion.h",
         "miro_hip_recursion_photons.h", "miro_hip_lens.h")
PATH = binding.MR_LEVEL_PATH


def header(name):
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", name)).read(), flags=re.S)


def test_the_four_symbols_are_exported_declared_and_bound(miro):
    """Fails on the parent commit: the symbols, the header and the eighth list are this feature's.  The seven older lists are as
    they were, and miro_hip.h alone reaches the new header (through miro_hip_lens.h, below its declarations)."""
    for name in NAMES:
        declared = lambda h: re.search(r"\bmr_status\s+%s\s*\(" % name, header(h)) is not None              # noqa: E731
        assert hasattr(miro.lib(), name) and getattr(miro.lib(), name).restype is C.c_int32
        assert declared("miro_hip_passes.h") and not any(declared(h) for h in OLDER)
        assert name not in (binding.LENS_SYMBOLS + binding.RECURSION_PHOTONS_SYMBOLS + binding.RECURSION_SYMBOLS + binding.RENDER_SYMBOLS +
                            binding.FRAME_SYMBOLS + binding.SURFACE_SYMBOLS + miro.EXPORTED_SYMBOLS)
    assert binding.PASSES_SYMBOLS == NAMES
    assert binding.LENS_SYMBOLS == ["mr_render_level_lights_lens", "mr_render_recursion_lens", "mr_render_recursion_photons_lens"]
    assert binding.RECURSION_PHOTONS_SYMBOLS == ["mr_render_recursion_photons_workspace", "mr_render_recursion_photons"]
    assert binding.RECURSION_SYMBOLS == ["mr_render_recursion_workspace", "mr_render_recursion"]
    assert binding.RENDER_SYMBOLS == ["mr_render_level_lights"]
    assert binding.FRAME_SYMBOLS == ["mr_render_lights_environment", "mr_trace_level_lights", "mr_trace_level_lights_path"]
    assert len(miro.EXPORTED_SYMBOLS) == 69 and len(binding.SURFACE_SYMBOLS) == 9
    raw = lambda h: open(os.path.join(ROOT, "include", h)).read().rstrip()                                  # noqa: E731
    assert raw("miro_hip.h").endswith('#include "miro_hip_render.h"\n#endif /* MIRO_HIP_H */')
    assert raw("miro_hip_lens.h").endswith('#include "miro_hip_passes.h"\n#endif /* MIRO_HIP_LENS_H */')
    assert raw("miro_hip_passes.h").endswith("#endif /* MIRO_HIP_PASSES_H */")
    for method in ("render_recursion_passes", "render_recursion_photons_passes", "finish_image"):
        assert hasattr(miro.Scene, method)
    from miro_amd import frame
    assert hasattr(frame.FrameRenderer, "finish")


def test_passes_desc_matches_the_header():
    """sizeof and the offsets, worked out from the header's own field list: eight 32-bit words and nothing else"""
    body = re.search(r"typedef struct mr_passes_desc \{(.*?)\} mr_passes_desc;", header("miro_hip_passes.h"), re.S).group(1)
    names, sizes = [], []
    for f in [f.strip() for f in body.split(";") if f.strip()]:
        assert f.startswith("uint32_t"), f
        for name in f[len("uint32_t"):].split(","):
            m = re.search(r"\[(\d+)\]", name)
            names.append(re.sub(r"\[\d+\]", "", name).strip())
            sizes.append(int(m.group(1)) if m else 1)
    D = binding.PassesDesc
    assert [n for n, _ in D._fields_] == names == ["spp_total", "sample_begin", "sample_end", "reserved"]
    assert C.sizeof(D) == 4 * sum(sizes) == 32
    off = 0
    for name, words in zip(names, sizes):
        assert getattr(D, name).offset == off and getattr(D, name).size == 4 * words
        off += 4 * words


def pdesc(S=8, begin=0, end=None, reserved=None):
    pd = binding.passes_desc(S, begin, end)
    if reserved is not None:
        pd.reserved[reserved] = 1
    return pd


def test_the_plan(miro):
    """whole passes of spp while they fit, then powers of two in descending order, from a begin that is a multiple of spp"""
    plan = binding.passes_plan
    assert plan(64, 1000) == [(64 * i, 64) for i in range(15)] + [(960, 32), (992, 8)]
    assert plan(4, 11) == [(0, 4), (4, 4), (8, 2), (10, 1)]
    assert plan(4, 7) == [(0, 4), (4, 2), (6, 1)]
    assert plan(1, 4) == [(0, 1), (1, 1), (2, 1), (3, 1)]
    assert plan(64, 64) == [(0, 64)]
    assert plan(64, 1000, 64, 128) == [(64, 64)]
    assert plan(64, 1000, 960, 1000) == [(960, 32), (992, 8)]
    assert plan(64, 1000, 0, 1) == [(0, 1)]
    for spp in (1, 2, 4, 8, 16, 32, 64):                                # every plan covers its range once, in order
        for S in (1, 3, 63, 64, 65, 127, 1000):
            p = plan(spp, S)
            assert p[0][0] == 0 and all(a + n == b for (a, n), (b, _) in zip(p, p[1:])) and p[-1][0] + p[-1][1] == S
            assert all(n <= spp and n & (n - 1) == 0 for _, n in p)
    L = miro.lib()
    n, base, size = C.c_uint32(99), (C.c_uint32 * 2)(7, 7), (C.c_uint32 * 2)(7, 7)
    assert L.mr_render_passes_plan(4, C.byref(pdesc(11)), C.byref(n), base, size, 2) == binding.MR_OK     # capacity cuts the lists
    assert n.value == 4 and list(base) == [0, 4] and list(size) == [4, 4]
    n.value = 99
    bad = [("NULL", (4, C.byref(pdesc()), None, base, size, 2)), ("NULL", (4, None, C.byref(n), base, size, 2)),
           ("spp", (3, C.byref(pdesc()), C.byref(n), base, size, 2)), ("spp", (128, C.byref(pdesc()), C.byref(n), base, size, 2)),
           ("spp", (0, C.byref(pdesc()), C.byref(n), base, size, 2)),
           ("reserved", (4, C.byref(pdesc(reserved=0)), C.byref(n), base, size, 2)),
           ("reserved", (4, C.byref(pdesc(reserved=4)), C.byref(n), base, size, 2)),
           ("spp_total", (4, C.byref(pdesc(S=0, end=0)), C.byref(n), base, size, 2)),
           ("range", (4, C.byref(pdesc(8, 4, 4)), C.byref(n), base, size, 2)), ("range", (4, C.byref(pdesc(8, 0, 9)), C.byref(n), base, size, 2)),
           ("multiple", (4, C.byref(pdesc(8, 2, 8)), C.byref(n), base, size, 2))]
    for word, args in bad:
        assert L.mr_render_passes_plan(*args) == binding.MR_ERR_INVALID, word
        msg = L.mr_last_error()
        assert word.encode() in msg and b"mr_render_passes_plan" in msg, (word, msg)
    assert n.value == 99 and list(base) == [0, 4]                       # a refused call writes nothing


def host_only_scene(miro):
    s = miro.Scene()
    s.add_triangle([0, 0, 0, 1, 0, 0, 0, 1, 0], [0, 0, 1] * 3)
    s.set_lights([dict(position=(0, 1, 0), wattage=5.0)])
    s.build(4, host_only=True)
    return s


@pytest.mark.parametrize("photons", [False, True], ids=["plain", "photons"])
def test_argument_errors_come_before_the_scene_and_the_device(miro, photons):
    """Every MR_ERR_INVALID case on a host_only one-triangle scene, answered from the arguments alone under this call's name: the
    parent call's list, the lens checks, then this call's own.  Then MR_ERR_STATE for that scene."""
    L = miro.lib()
    s = host_only_scene(miro)
    who = b"mr_render_recursion_photons_passes" if photons else b"mr_render_recursion_passes"
    p = lambda a: C.c_void_p(a)                                                   # noqa: E731
    fd0 = frame_desc(binding)
    need = C.c_uint64(0)
    if photons:
        assert L.mr_render_recursion_photons_workspace(C.byref(fd0), C.byref(rdesc()), C.byref(need)) == binding.MR_OK
    need = need.value if photons else workspace(100, False, 0)
    base = dict(scene=s.h, lens=None, rgb=p(8192), ws=p(1 << 20), bytes=1 << 40, counts=p(1 << 16), maps=(p(4096), None), k=50, dist=1.0)

    def call(fd, rd, pd, **kw):
        a = dict(base, **kw)
        ref = lambda d: C.byref(d) if d is not None else None                     # noqa: E731
        extra = (a["maps"][0], a["maps"][1], a["dist"], a["k"]) if photons else ()
        fn = L.mr_render_recursion_photons_passes if photons else L.mr_render_recursion_passes
        st = fn(a["scene"], ref(fd), ref(a["lens"]), ref(rd), ref(pd), *extra, a["rgb"], a["ws"], a["bytes"], a["counts"], None)
        return st, L.mr_last_error()

    fd, ok, pd = frame_desc(binding), rdesc(), pdesc(8, 0, 8)
    spp4 = frame_desc(binding, spp=4)
    tiled = frame_desc(binding, spp=4)
    tiled.tiled = 1
    big = frame_desc(binding, W=65536, H=65536, y1=1)                              # 65536 pixels in the window
    invalid = [
        # the parent call's list
        ("NULL", call(fd, ok, pd, scene=None)), ("NULL", call(None, ok, pd)), ("NULL", call(fd, ok, pd, rgb=None)),
        ("empty image", call(frame_desc(binding, W=0), ok, pd)), ("spp", call(frame_desc(binding, spp=3), ok, pd)),
        ("flags", call(frame_desc(binding, flags=binding.MR_TRACE_ANY), ok, pd)),
        ("aligned", call(fd, ok, pd, rgb=p(8194))), ("aligned", call(fd, ok, pd, counts=p((1 << 16) + 4))),
        ("NULL", call(fd, None, pd)), ("d_pass_counts", call(fd, ok, pd, counts=None)),
        ("depth", call(fd, rdesc(depth=65), pd)), ("children", call(fd, rdesc(children=0), pd)),
        ("environment", call(fd, rdesc(environment=2), pd)), ("path_kinds", call(fd, rdesc(children=PATH, kinds=0), pd)),
        ("reserved", call(fd, rdesc(reserved=0), pd)), ("queue_capacity", call(fd, rdesc(capacity=0), pd)),
        ("workspace", call(fd, ok, pd, ws=None)), ("workspace", call(fd, ok, pd, ws=p((1 << 20) + 8))),
        ("workspace_bytes", call(fd, ok, pd, bytes=need - 1)),
        # the lens checks, with a lens
        ("mr_lens_desc.reserved", call(fd, ok, pd, lens=lens_desc(reserved=0))), ("aperture", call(fd, ok, pd, lens=lens_desc(aperture=-1.0))),
        ("focus_plane", call(fd, ok, pd, lens=lens_desc(focus_plane=0.0))),
        # this call's own
        ("tiled", call(tiled, ok, pd)), ("tiled", call(tiled, ok, pd, lens=lens_desc())),
        ("NULL argument (passes)", call(fd, ok, None)),
        ("mr_passes_desc.reserved", call(fd, ok, pdesc(reserved=0))), ("mr_passes_desc.reserved", call(fd, ok, pdesc(reserved=4))),
        ("spp_total", call(fd, ok, pdesc(S=0, end=0))),
        ("range", call(fd, ok, pdesc(8, 3, 3))), ("range", call(fd, ok, pdesc(8, 5, 4))), ("range", call(fd, ok, pdesc(8, 0, 9))),
        ("multiple", call(spp4, ok, pdesc(8, 2, 8))), ("multiple", call(spp4, ok, pdesc(16, 6, 8))),
        ("ray ids", call(big, ok, pdesc(65536, 0, 1))),
    ]
    if photons:
        invalid += [("global_map and caustic_map", call(fd, ok, pd, maps=(None, None))), ("nphotons", call(fd, ok, pd, k=0)),
                    ("max_dist", call(fd, ok, pd, dist=0.0)), ("workspace", call(fd, rdesc(depth=0, children=0, capacity=0), pd, ws=None))]
    for word, (st, msg) in invalid:
        assert st == binding.MR_ERR_INVALID, (word, st, msg)
        assert word.encode() in msg and who in msg and b"HIP device" not in msg and b"host_only" not in msg, (word, msg)
    good = [call(fd, ok, pd), call(fd, ok, pd, lens=lens_desc()), call(spp4, ok, pdesc(1000, 64 * 4, 1000)),
            call(big, rdesc(depth=0, children=0, capacity=0), pdesc(65536, 0, 1)),                       # depth 0: no ids, no limit
            call(big, ok, pdesc(65535, 0, 1)), call(fd, ok, pd, bytes=need)]
    for st, msg in good:                                                          # then the scene's state: never a CPU path
        assert st == binding.MR_ERR_STATE and (b"CPU" in msg or b"device" in msg) and b"HIP device" not in msg, msg
    assert s.info().n_triangles == 1                                              # the refused calls left the scene alone


def test_finish_image_refusals(miro):
    L = miro.lib()
    s = host_only_scene(miro)
    p = lambda a: C.c_void_p(a)                                                   # noqa: E731
    bad = [("NULL", (None, p(4096), 4, p(8192), None, None)), ("NULL", (s.h, None, 4, p(8192), None, None)),
           ("NULL", (s.h, p(4096), 4, None, None, None)), ("empty image", (s.h, p(4096), 0, p(8192), None, None)),
           ("2^32", (s.h, p(4096), 1 << 32, p(8192), None, None)), ("aligned", (s.h, p(4098), 4, p(8192), None, None)),
           ("aligned", (s.h, p(4096), 4, p(8192), p(12290), None))]
    for word, args in bad:
        assert L.mr_finish_image(*args) == binding.MR_ERR_INVALID, word
        msg = L.mr_last_error()
        assert word.encode() in msg and b"mr_finish_image" in msg, (word, msg)


def test_samples_needs_a_device_route():
    """render_specular(samples=...) on a route that is not "device_*" raises before anything is launched"""
    import torch
    from miro_amd import frame
    from test_frame_plan import DESC, LIGHTS, SCENES, RecordingScene
    sc = RecordingScene(*SCENES["plain"], hit=(3, 4), child=(1, 2), image=False)
    fr = frame.FrameRenderer(sc, DESC, 16, 8, spp=2, device=torch.device("cpu"), resident_rays=False)
    for fused in (False, True, "auto", "lights", "frame_lights", "frame_lens"):
        with pytest.raises(ValueError) as e:
            fr.render_specular(depth=1, lights=LIGHTS, fused=fused, samples=8)
        assert "samples" in str(e.value) and "device_" in str(e.value)
    assert sc.calls == []


def test_pass_kernels_stay_inside_the_verified_envelope():
    """Every kernel of mr_frame_passes.hip: 36 frame kernels (six traversal variants x CHILDREN 0 / 1 / 2 x pinhole / lens) and the
    two query kernels; no dynamic stack, no spilled VGPR, at least four waves per SIMD; no more spilled VGPRs, no more scratch per
    lane and no fewer waves than BOTH its own record (tests/golden/kernel_budget_frame_passes.json, written from the build whose
    GPU suite was green) AND the worst value among the kernels of tests/golden/kernel_budget.json.  The two kernels of
    mr_finish_image.hip likewise, against tests/golden/kernel_budget_finish_image.json."""
    cur = kernel_budget.unit_kernels("mr_frame_passes")
    frame_kernels = [k for k in cur if "frame_pass_kernel" in k]
    assert len(frame_kernels) == 36 and len(cur) == 38
    for var in (1818, 826, 267, 43, 88, 73):
        for ch in (0, 1, 2):
            for lens in (0, 1):
                assert sum("frame_pass_kernelILi%dELi%dELb%dEE" % (var, ch, lens) in k for k in cur) == 1, (var, ch, lens)
    assert sum("gather_eye_queries_pass_kernel" in k for k in cur) == 2
    assert all(v["vgprs_spilled"] == 0 and v["waves_per_simd"] >= 4 for v in cur.values())
    kernel_budget.assert_inside_envelope(cur, "kernel_budget_frame_passes.json", also_main=True)
    fin = kernel_budget.unit_kernels("mr_finish_image")
    assert sorted(k.split("_GLOBAL__N_1")[1][2:].split("E")[0] for k in fin) == ["finish_map_kernel", "finish_minmax_kernel"]
    assert all(v["vgprs_spilled"] == 0 and v["scratch_bytes_per_lane"] == 0 for v in fin.values())
    kernel_budget.assert_inside_envelope(fin, "kernel_budget_finish_image.json", also_main=True)
