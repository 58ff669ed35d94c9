"""mr_render_recursion on the MI355X (include/miro_hip_recursion.h, csrc/mr_level_lights_queued.hip): the whole recursive frame as
one call whose level kernels read the length of their queue from the device.

The yardstick of every comparison is render_specular(fused="frame_lights" | "frame_lights_path") with the same FrameRenderer
arguments: existing code, whose level 0 is the same launch and whose further levels are mr_trace_level_lights[_path] with the
queue's length read back to the host.  A FrameRenderer subclass keeps what that route computes on its way -- the six counters of
every level and the pixel column of every queue -- so that the counters can be compared word for word and the precondition of the
bit-for-bit comparisons (no pixel twice in a level's queue) is asserted from the yardstick's own queues.

  counts      words 0..5 of every level EXACTLY; a level's children are the next level's rays
  pixels      bit for bit where every pixel receives at most one addition per level (mirror-only scene, 1 spp); elsewhere
              rtol = 1e-5, atol = 1e-6 x max|rgb|, the bound tests/test_level_lights.py holds float-atomic pixel sums to
  windows     24 x 16 and 40 x 24 at 1 and 4 spp: 384 to 3 840 samples, more than one workgroup each; at 1 spp the samples are no
              multiple of 256, and every case has child counts that are none (asserted); depth 3"""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_frame_level_lights import GLASS_DESC  # noqa: E402
from test_frame_lights import bits, camera  # noqa: E402
from test_frame_lights_surface import scene_of  # noqa: E402
from test_level_lights import ENVS, use  # noqa: E402
from test_level_lights_path import glass_sphere  # noqa: E402

SPECULAR, PATH = 1, 2                                   # MR_LEVEL_SPECULAR, MR_LEVEL_PATH
MIRROR_ONLY = 1                                         # MR_PATH_MIRROR
WINDOWS = {1: (40, 24), 4: (24, 16)}                    # spp -> (W, H)
DEPTH = 3
SEED = 29
GLASS_LIGHTS = [dict(position=(3.0, 4.0, 5.0), wattage=50.0)]
MIRROR_DESC = dict(eye=(0.0, 1.6, 6.0), lookat=(0.0, 0.8, 0.0), up=(0.0, 1.0, 0.0), fov=40.0)
MIRROR_LIGHTS = [dict(position=(3.0, 5.0, 4.0), wattage=120.0), dict(position=(-4.0, 3.0, 2.0), color=(1.0, 0.8, 0.6), wattage=60.0)]
_OWN = {}


def mirror_scene(miro):
    """two mirror spheres (ks = 0.8, kt = 0) that see each other over a floor and a back wall that reflect a little (ks = 0.3):
    every hit has exactly one child, the reflection, so a pixel's sample has one ray per level"""
    s = miro.Scene(0)
    s.add_triangle([-30, 0, 30, 30, 0, 30, 0, 0, -30], [0, 1, 0] * 3)
    s.add_triangle([-30, 0, -4, 30, 0, -4, 0, 40, -4], [0, 0, 1] * 3)
    s.add_sphere((-1.1, 1.0, 0.0), 1.0)
    s.add_sphere((1.1, 1.0, 0.3), 1.0)
    s.set_materials([((0.6, 0.5, 0.4), (0.3, 0.3, 0.3), (0, 0, 0), 40.0, 1.0), ((0.1, 0.1, 0.1), (0.8, 0.8, 0.8), (0, 0, 0), 200.0, 1.0)],
                    [0, 0, 1, 1])
    s.build(4)
    return s


def scene(miro, name, env):
    """(scene, description, lights) with the lights and the environment ENVS[env] set"""
    if name in ("flower_drops",):
        return use(miro, name, env)
    if name == "teapot":
        s, desc, lights = scene_of(miro, name)
    else:
        if name not in _OWN:
            _OWN[name] = glass_sphere(miro) if name == "glass" else mirror_scene(miro)
        s, desc, lights = _OWN[name], (GLASS_DESC if name == "glass" else MIRROR_DESC), (GLASS_LIGHTS if name == "glass" else MIRROR_LIGHTS)
    s.set_lights(lights)
    s.set_environment(**(ENVS[env] or {}))
    return s, desc, lights


def frames(miro, name, env, children, spp, kinds=7, depth=DEPTH, capacity=None, device=True, window=None, own=None):
    """The yardstick frame and the frame under test with the same arguments.  Returns (ref, dev): each with per_level, rgb and
    counts [levels, 6+]; ref besides with pixels, the pixel column of every queue it ran (levels >= 1).
    own: (scene, description, lights, environment) of a caller's own scene, the environment as the arguments of
    Scene.set_environment or None -- `name` and `env` are then not looked at."""
    import torch
    from miro_amd import frame

    class Spy(frame.FrameRenderer):
        def _level_buffers(self, plan, n, level, last):
            out = super()._level_buffers(plan, n, level, last)
            self.seen_counts.append(out[2])
            return out

        def _level_lights(self, plan, q, level, last, rgb=None):
            self.seen_pixels.append(q.pixels)
            return super()._level_lights(plan, q, level, last, rgb=rgb)

    if own is None:
        s, desc, lights = scene(miro, name, env)
        environment = ENVS[env]
    else:
        s, desc, lights, environment = own
        s.set_lights(lights)
        s.set_environment(**(environment or {}))
    w, h = window or WINDOWS[spp]
    kw = dict(depth=depth, lights=lights, environment=environment)
    if children == PATH:
        kw.update(path_tracing=True, path_kinds=kinds, path_seed=SEED)
    route = "lights_path" if children == PATH else "lights"
    ref = Spy(s, desc, w, h, spp=spp, tiled=False, resident_rays=False)
    ref.seen_counts, ref.seen_pixels = [], []
    ref.per_level = ref.render_specular(fused="frame_" + route, **kw)
    torch.cuda.synchronize()
    ref.counts = [c.tolist() for c in ref.seen_counts]
    ref.pixels = [p.cpu().numpy() for p in ref.seen_pixels]
    ref.rgb = ref.d_rgb.clone()
    if not device:
        return ref, None
    dev = frame.FrameRenderer(s, desc, w, h, spp=spp, tiled=False, resident_rays=False)
    dev.per_level = dev.render_specular(fused="device_" + route, queue_capacity=capacity, **kw)
    torch.cuda.synchronize()
    dev.counts = dev.d_level_counts[:depth + 1].tolist()
    dev.rgb = dev.d_rgb.clone()
    return ref, dev


def assert_counts(ref, dev, depth=DEPTH):
    """words 0..5 of every level the yardstick ran; the levels it did not run are all-zero rows; words 6 and 7 are 0; a level's
    children are the next level's rays"""
    assert len(dev.counts) == depth + 1 and all(len(row) == 8 for row in dev.counts)
    for level, row in enumerate(dev.counts):
        want = ref.counts[level][:6] if level < len(ref.counts) else [0] * 6
        assert row[:6] == want, (level, row, want)
        assert row[6:] == [0, 0]
        if level < depth:
            assert dev.counts[level + 1][0] == row[5]
    assert dev.per_level == ref.per_level


def assert_pixels_close(ref, dev):
    import torch
    scale = float(ref.rgb.abs().max())
    assert scale > 0
    assert torch.allclose(dev.rgb, ref.rgb, rtol=1e-5, atol=1e-6 * scale), float((dev.rgb - ref.rgb).abs().max())


@pytest.mark.gpu
@pytest.mark.parametrize("env", [None, "colour", "image"])
@pytest.mark.parametrize("children", [SPECULAR, PATH], ids=["specular", "path"])
@pytest.mark.parametrize("spp", [1, 4])
@pytest.mark.parametrize("window", [(24, 16), (40, 24)], ids=["24x16", "40x24"])
@pytest.mark.parametrize("name", ["glass", "flower_drops", "mirror"])
def test_counts_exactly_and_pixels_within_the_atomic_bound(miro, name, window, spp, children, env):
    ref, dev = frames(miro, name, env, children, spp, window=window)
    print("per_level", ref.per_level, "counts", ref.counts)
    assert len(ref.per_level) == DEPTH + 1 and all(n > 0 for n, _ in ref.per_level)      # the case runs every level
    assert ref.counts[0][0] == window[0] * window[1] * spp and (spp > 1 or ref.counts[0][0] % 256 != 0)
    assert any(row[5] % 256 != 0 for row in ref.counts[:DEPTH])
    assert_counts(ref, dev)
    assert_pixels_close(ref, dev)


@pytest.mark.gpu
@pytest.mark.parametrize("env", [None, "colour"])
@pytest.mark.parametrize("children", [SPECULAR, PATH], ids=["specular", "path"])
def test_mirror_only_at_one_sample_is_the_yardsticks_bits(miro, children, env):
    """One ray per pixel and level: the precondition is asserted from the yardstick's own queues, then d_rgb is compared on its
    bits (level 0 is a store, every further level one float add per pixel, the levels ordered by the stream)."""
    ref, dev = frames(miro, "mirror", env, children, 1, kinds=MIRROR_ONLY)
    assert len(ref.pixels) == DEPTH and len(ref.pixels[0]) > 256 and all(len(p) > 0 for p in ref.pixels)     # level 1: several workgroups
    for level, p in enumerate(ref.pixels, 1):
        assert len(np.unique(p)) == len(p), level
    assert_counts(ref, dev)
    assert np.array_equal(bits(dev.rgb), bits(ref.rgb))


@pytest.mark.gpu
@pytest.mark.parametrize("name,env", [("flower_drops", "image"), ("glass", None), ("mirror", "colour")])
def test_depth_0_is_the_level_0_frame_bit_for_bit(miro, name, env):
    """mr_render_lights_environment (without an environment: mr_render_lights_surface) with its five counters; no workspace"""
    import torch
    s, desc, lights = scene(miro, name, env)
    w, h = WINDOWS[4]
    n_pix = w * h
    rgb = torch.full((n_pix, 3), 7.0, dtype=torch.float32, device="cuda")
    want = torch.full((n_pix, 3), 9.0, dtype=torch.float32, device="cuda")
    counts = torch.full((1, 8), 999, dtype=torch.int64, device="cuda")
    five = torch.zeros(5, dtype=torch.int64, device="cuda")
    s.render_recursion(camera(desc), w, h, rgb, counts, 0, spp=4, jitter=True, environment=env is not None, children=0)
    if env is not None:
        s.render_lights_environment(camera(desc), w, h, want, spp=4, jitter=True, d_counts=five)
    else:
        s.render_lights_surface(camera(desc), w, h, want, spp=4, jitter=True, d_counts=five[:3])
    torch.cuda.synchronize()
    assert np.array_equal(bits(rgb), bits(want)) and float(want.abs().max()) > 0
    got = counts[0].tolist()
    assert got[5:] == [0, 0, 0] and got[:3] == five.tolist()[:3] and got[0] == n_pix * 4
    if env is not None:
        assert got[:5] == five.tolist()
    else:
        assert got[3] > 0 and got[4] == 0               # the open scene's misses are counted without an environment too


@pytest.mark.gpu
def test_a_queue_that_dies_out(miro):
    """the plain teapot has no specular material: levels >= 1 are all-zero rows, d_rgb is level 0's bits, one entry comes back"""
    import torch
    ref, dev = frames(miro, "teapot", None, SPECULAR, 4)
    assert len(ref.per_level) == 1 and dev.per_level == ref.per_level
    assert dev.counts[0][:6] == ref.counts[0][:6] and dev.counts[0][5] == 0 and dev.counts[0][1] > 0
    assert dev.counts[1:] == [[0] * 8] * DEPTH
    assert np.array_equal(bits(dev.rgb), bits(ref.rgb)) and float(ref.rgb.abs().max()) > 0
    s, desc, lights = scene(miro, "teapot", None)
    w, h = WINDOWS[4]
    zero = torch.zeros((w * h, 3), dtype=torch.float32, device="cuda")
    s.render_lights_surface(camera(desc), w, h, zero, spp=4, jitter=True)
    torch.cuda.synchronize()
    assert np.array_equal(bits(dev.rgb), bits(zero))


@pytest.mark.gpu
def test_a_capacity_of_100_truncates_inside_the_declared_workspace(miro):
    """Level 0 of the glass sphere at 24 x 16 x 4 emits more than 100 children (asserted on the yardstick).  With queue_capacity =
    100 the call is MR_OK, [0][5] is the true count, level 1 runs exactly 100 rays, and the guard regions in front of and behind
    the declared workspace keep their pattern.  render_specular raises RuntimeError.  Once: a bounds check."""
    import torch
    from miro_amd import frame
    ref, _ = frames(miro, "glass", "colour", PATH, 4, device=False)
    true_children = ref.counts[0][5]
    assert true_children > 100
    s, desc, lights = scene(miro, "glass", "colour")
    w, h = WINDOWS[4]
    need = s.recursion_workspace_bytes(DEPTH, 100, children=PATH, environment=True)
    guard = 4096
    buf = torch.full((guard + need + guard,), 0xA5, dtype=torch.uint8, device="cuda")
    rgb = torch.zeros((w * h, 3), dtype=torch.float32, device="cuda")
    counts = torch.zeros((DEPTH + 1, 8), dtype=torch.int64, device="cuda")
    s.render_recursion(camera(desc), w, h, rgb, counts, DEPTH, d_workspace=buf[guard:guard + need], queue_capacity=100, spp=4, jitter=True,
                       children=PATH, environment=True, kinds=7, path_seed=SEED)       # raises unless MR_OK
    torch.cuda.synchronize()
    got = counts.tolist()
    assert got[0][:6] == ref.counts[0][:6] and got[0][5] == true_children
    assert got[1][0] == 100 and all(row[0] <= 100 for row in got[1:])
    assert bool((buf[:guard] == 0xA5).all()) and bool((buf[guard + need:] == 0xA5).all())
    assert not bool((buf[guard:guard + need] == 0xA5).all())                            # the queues were written
    fr = frame.FrameRenderer(s, desc, w, h, spp=4, tiled=False, resident_rays=False)
    with pytest.raises(RuntimeError) as e:
        fr.render_specular(depth=DEPTH, lights=lights, environment=ENVS["colour"], path_tracing=True, path_kinds=7, path_seed=SEED,
                           fused="device_lights_path", queue_capacity=100)
    assert "level 0" in str(e.value) and str(true_children) in str(e.value) and "100" in str(e.value)


@pytest.mark.gpu
@pytest.mark.parametrize("name,children,kinds", [("mirror", SPECULAR, 7), ("glass", PATH, 7)])
def test_replays_from_a_captured_graph(miro, name, children, kinds):
    """After one direct call (it uploads what the scene needs) one mr_render_recursion is captured into a torch.cuda.graph on one
    stream -- a linear graph -- and replayed twice into the same d_rgb and counters, both filled with wrong values before each
    replay: the counters are the direct call's (the zeroing kernel replays), and on the mirror-only scene at 1 spp so are the bits."""
    import torch
    s, desc, lights = scene(miro, name, "colour")
    spp = 1 if name == "mirror" else 4
    w, h = WINDOWS[spp]
    cap = 4 * w * h * spp
    ws = torch.empty(s.recursion_workspace_bytes(DEPTH, cap, children=children, environment=True), dtype=torch.uint8, device="cuda")
    rgb = torch.zeros((w * h, 3), dtype=torch.float32, device="cuda")
    counts = torch.zeros((DEPTH + 1, 8), dtype=torch.int64, device="cuda")

    def launch(stream):
        s.render_recursion(camera(desc), w, h, rgb, counts, DEPTH, d_workspace=ws, queue_capacity=cap, spp=spp, jitter=spp > 1,
                           children=children, environment=True, kinds=kinds, path_seed=SEED, stream=stream)

    launch(None)
    torch.cuda.synchronize()
    want_counts, want_rgb = counts.tolist(), rgb.clone()
    assert all(row[0] > 0 for row in want_counts) and want_counts[0][5] % 256 != 0
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
        if name == "mirror":
            assert np.array_equal(bits(rgb), bits(want_rgb))
        else:
            assert torch.allclose(rgb, want_rgb, rtol=1e-5, atol=1e-6 * float(want_rgb.abs().max()))


@pytest.mark.gpu
@pytest.mark.parametrize("children", ["specular", "path"])
def test_the_c_program_renders_the_recursive_frame_without_python(tmp_path, miro, children):
    """tests/cpp/abi_recursion.cpp, g++ only: exits 0, and the counters it prints are the Python call's on the same scene"""
    import torch
    exe = str(tmp_path / "abi_recursion")
    lib_dir = os.path.dirname(miro.lib_path())
    subprocess.check_call(["g++", "-std=c++11", "-O1", "-Wall", "-Wextra", "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(ROOT, "include"),
                           "-I", "/opt/rocm/include", os.path.join(ROOT, "tests", "cpp", "abi_recursion.cpp"),
                           "-L", lib_dir, "-lmiro_hip", "-L", "/opt/rocm/lib", "-lamdhip64",
                           "-Wl,-rpath," + lib_dir, "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    w, h = WINDOWS[4]
    out = subprocess.run([exe, str(w), str(h), "4", str(DEPTH), children, "0"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert out.returncode == 0, out.stderr.decode()
    lines = out.stdout.decode().split("\n")
    printed = [[int(v) for v in ln.split()[2:]] for ln in lines if ln.startswith("level ")]
    assert not any(ln.startswith("truncated") for ln in lines) and any(ln.startswith("checksum ") for ln in lines)
    s, desc, lights = scene(miro, "glass", None)
    kind = PATH if children == "path" else SPECULAR
    cap = (4 if kind == PATH else 3) * w * h * 4
    ws = torch.empty(s.recursion_workspace_bytes(DEPTH, cap, children=kind), dtype=torch.uint8, device="cuda")
    rgb = torch.zeros((w * h, 3), dtype=torch.float32, device="cuda")
    counts = torch.zeros((DEPTH + 1, 8), dtype=torch.int64, device="cuda")
    s.render_recursion(camera(desc), w, h, rgb, counts, DEPTH, d_workspace=ws, queue_capacity=cap, spp=4, jitter=True, children=kind,
                       kinds=7, path_seed=168)
    torch.cuda.synchronize()
    assert printed == counts.tolist() and all(row[0] > 0 for row in printed)
