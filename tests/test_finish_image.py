"""mr_finish_image on the MI355X (include/miro_hip_passes.h, csrc/mr_finish_image.hip): Scene.cpp:150-163, 184-197 and Image.cpp:47-52 --
the image's maximum and minimum over its non-NaN channel values, every NaN channel replaced by that maximum, then mr_tonemap's
bytes.

The yardstick is mr_tonemap itself (unchanged) on the same image with the NaNs replaced on the host by numpy.nanmax (-inf where
the image has no number), so the bytes are compared bit for bit; d_minmax is compared with numpy.nanmax / numpy.nanmin on its bits.
Images of 1, 255, 257 and 24 x 16 pixels: less than a wave, one value short of and one value past three workgroups of 256
values, and several workgroups.  The state words the two kernels share are put back by the call itself: every case runs twice."""
import os
import sys
import warnings

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

SIZES = [1, 255, 257, 24 * 16]
KINDS = ["no_nan", "scattered", "all_nan", "inf", "negative"]


def image(kind, n, seed):
    rng = np.random.default_rng(seed)
    a = rng.uniform(0.01, 1.5, size=(n, 3)).astype(np.float32)
    if kind == "scattered":
        a[rng.random((n, 3)) < 0.2] = np.nan
        a[0, 1] = np.nan                                # at least one, also in the 1-pixel image, and one number beside it
    elif kind == "all_nan":
        a[:] = np.nan
    elif kind == "inf":
        a[rng.random((n, 3)) < 0.1] = np.nan
        a[n // 2, 2] = np.inf
        a[0, 0] = np.nan
    elif kind == "negative":
        a = -a
        a[rng.random((n, 3)) < 0.1] = np.nan
    return a


def nan_max_min(a):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        hi, lo = np.nanmax(a), np.nanmin(a)
    return (np.float32(-np.inf) if np.isnan(hi) else np.float32(hi)), (np.float32(np.inf) if np.isnan(lo) else np.float32(lo))


def finish_and_yardstick(scene, a):
    """(bytes of mr_finish_image, d_minmax, bytes of mr_tonemap on the image with NaN -> nanmax)"""
    import torch
    n = a.shape[0]
    hi, _ = nan_max_min(a)
    filled = np.where(np.isnan(a), hi, a).astype(np.float32)
    d_rgb = torch.from_numpy(a).cuda()
    d_out = torch.full((n, 3), 77, dtype=torch.uint8, device="cuda")
    d_minmax = torch.full((2,), 5.0, dtype=torch.float32, device="cuda")
    d_want = torch.full((n, 3), 78, dtype=torch.uint8, device="cuda")
    scene.finish_image(d_rgb, n, d_out, d_minmax=d_minmax)
    scene.tonemap(torch.from_numpy(filled).cuda(), 3 * n, d_want)
    torch.cuda.synchronize()
    assert d_rgb.cpu().numpy().tobytes() == a.tobytes()                # the image is not changed
    return d_out.cpu().numpy(), d_minmax.cpu().numpy(), d_want.cpu().numpy()


@pytest.fixture(scope="module")
def any_scene(miro):
    s = miro.Scene(0)
    s.add_triangle([0, 0, 0, 1, 0, 0, 0, 1, 0], [0, 0, 1] * 3)
    s.build(4)
    return s


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n", SIZES)
def test_bytes_are_tonemaps_and_minmax_is_nanmax_nanmin(any_scene, n, kind):
    for run in range(2):                                                # the second call starts from the state the first put back
        a = image(kind, n, 100 * n + run)
        got, minmax, want = finish_and_yardstick(any_scene, a)
        hi, lo = nan_max_min(a)
        print(kind, n, "max", hi, "min", lo, "nan channels", int(np.isnan(a).sum()))
        assert minmax.view(np.uint32).tolist() == [hi.view(np.uint32), lo.view(np.uint32)], (minmax, hi, lo)
        assert np.array_equal(got, want)
        if kind == "all_nan":
            assert hi == -np.inf and not got.any()                      # maximum -inf: all zero bytes
        if kind == "inf":
            assert hi == np.inf and (got[np.isnan(a)] == 255).all()
        if kind == "negative":
            assert hi < 0 and lo < hi


@pytest.mark.gpu
def test_minmax_is_optional_and_the_renderer_returns_the_bytes(miro, any_scene):
    import torch
    from miro_amd import frame
    a = image("scattered", 257, 7)
    d_out = torch.zeros((257, 3), dtype=torch.uint8, device="cuda")
    any_scene.finish_image(torch.from_numpy(a).cuda(), 257, d_out)
    _, _, want = finish_and_yardstick(any_scene, a)
    assert np.array_equal(d_out.cpu().numpy(), want)
    desc = dict(eye=(0.3, 0.3, 3.0), lookat=(0.3, 0.3, 0.0), up=(0.0, 1.0, 0.0), fov=40.0)
    fr = frame.FrameRenderer(any_scene, desc, 24, 16, resident_rays=False)
    fr.d_rgb.copy_(torch.from_numpy(image("scattered", 24 * 16, 8)).cuda())
    out = fr.finish()
    _, _, want = finish_and_yardstick(any_scene, fr.d_rgb.cpu().numpy())
    assert out.dtype == torch.uint8 and tuple(out.shape) == (24 * 16, 3) and np.array_equal(out.cpu().numpy(), want)
    assert fr.finish().data_ptr() == out.data_ptr()                    # the renderer keeps the buffer


@pytest.mark.gpu
def test_a_fuzz_frame_with_nan_pixels(oracle, miro):
    """A frame of tests/test_lights_fuzz.py's scenes (a tenth of the triangles have zero vertex normals: NaN hit normals, NaN
    pixels), rendered as three one-sample passes at depth 2 and finished: the first view that holds a NaN pixel and a number.
    No byte depends on the NaNs beyond the rule -- the bytes are mr_tonemap's on the image with its NaNs replaced by nanmax."""
    import torch
    from miro_amd import binding
    import test_lights_fuzz as LF
    from test_frame_lights import camera
    for seed in range(LF.SEEDS):
        case = LF.case_of(oracle, seed)
        scene = LF.product_of(miro, case, textured=True)
        scene.set_lights(case.lights)
        env = case.environment_args() or None
        scene.set_environment(**(env or {}))
        for v in case.views:
            w, h, cap = v["W"], v["H"], 9 * v["W"] * v["H"]
            rgb = torch.zeros((w * h, 3), dtype=torch.float32, device="cuda")
            counts = torch.zeros((3, 3, 8), dtype=torch.int64, device="cuda")
            ws = torch.empty(max(scene.recursion_workspace_bytes(2, cap, environment=env is not None), 16), dtype=torch.uint8, device="cuda")
            scene.render_recursion_passes(camera(v["desc"]), w, h, rgb, counts, 2, 3, d_workspace=ws, queue_capacity=cap, spp=1,
                                          jitter=True, environment=env is not None, children=binding.MR_LEVEL_SPECULAR)
            torch.cuda.synchronize()
            a = rgb.cpu().numpy()
            nans = int(np.isnan(a).sum())
            if nans == 0 or nans == a.size:
                continue
            got, minmax, want = finish_and_yardstick(scene, a)
            hi, lo = nan_max_min(a)
            print("seed", seed, "window", w, h, "nan channels", nans, "max", hi, "min", lo)
            assert minmax.view(np.uint32).tolist() == [hi.view(np.uint32), lo.view(np.uint32)]
            assert np.array_equal(got, want)
            scene.set_environment()
            return
        scene.set_environment()
    pytest.fail("no fuzz view rendered a frame with both NaN pixels and numbers")
