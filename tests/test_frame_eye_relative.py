"""The fused frame's primary trace on eye-relative tables (mr_frame.hip: eye_tables, trace_ray's REL): node corners, root box
and the origin terms of every triangle test are computed once per call relative to the camera eye, and the primary rays are
traced from a zero origin.  The same fp32 operations on the same operands, so the hit records and the picture must be the
batched pipeline's (which traces on the scene's own tables) bit for bit -- for every eye, including eyes on a slab plane,
inside the root box, with a zero component and with a component outside the regular range (the true-division path)."""
import numpy as np
import pytest
import torch

from helpers import product_scene
from miro_amd import frame as mframe
from miro_amd import scenes

pytestmark = pytest.mark.gpu


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32).numpy()


def _desc(name, eye=None):
    d = dict(scenes.SCENES[name])
    if eye is not None:
        d["eye"] = tuple(float(np.float32(v)) for v in eye)
    return d


def _compare(sc, d, W, H, spp, tiled=False, any_shadow=False):
    """fused frame (eye-relative primary trace) against the batched pipeline: primary records, shadow records, counts, rgb"""
    ref = mframe.FrameRenderer(sc, d, W, H, spp=spp, tiled=tiled)
    ref.generate()
    ref.step(any_hit=any_shadow)
    fu = mframe.FusedFrame(sc, d, W, H, spp=spp, tiled=tiled, keep_hits=True, any_shadow=any_shadow)
    fu.step()
    torch.cuda.synchronize()
    n_p, n_s = ref.ray_counts()
    assert fu.ray_counts() == (n_p, n_s)
    assert np.array_equal(_bits(fu.d_hits), _bits(ref.d_hits))
    src = ref.d_src[:n_s].to(torch.int64)
    assert np.array_equal(_bits(fu.d_shadow_hits[src]), _bits(ref.d_shadow_hits[:n_s]))
    assert np.array_equal(_bits(fu.d_rgb), _bits(ref.d_rgb))
    return fu, ref


def _root_box(sc):
    corners, _, _ = sc.export_tree()
    return corners[0, :3], corners[0, 3:]


def _slab_eye(sc, eye):
    """the eye moved onto the nearest slab planes of the tree: x and y of node corners (relative corner exactly 0)"""
    corners, _, _ = sc.export_tree()
    fin = corners[np.isfinite(corners).all(axis=1)]
    e = list(np.float32(eye))
    for k in (0, 1):
        vals = np.concatenate([fin[:, k], fin[:, 3 + k]])
        e[k] = vals[np.argmin(np.abs(vals - e[k]))]
    return e


@pytest.mark.parametrize("name,W,H,spp,tiled", [
    ("teapot", 96, 64, 1, True), ("teapot", 40, 30, 64, False), ("bunny", 80, 45, 4, True), ("bunny", 33, 21, 64, False),
    ("sponza", 120, 67, 1, False), ("sponza", 64, 36, 4, True), ("sponza", 48, 27, 64, False), ("cornell", 33, 31, 4, True),
    ("cornell", 64, 64, 1, False)])
def test_scene_eye(miro, name, W, H, spp, tiled):
    sc = product_scene(miro, name)
    _compare(sc, _desc(name), W, H, spp, tiled)


@pytest.mark.parametrize("name", ["sponza", "teapot", "bunny"])
@pytest.mark.parametrize("kind", ["slab", "zero", "irregular", "tiny_negative"])
def test_special_eyes(miro, name, kind):
    sc = product_scene(miro, name)
    eye = list(scenes.SCENES[name]["eye"])
    if kind == "slab":
        eye = _slab_eye(sc, eye)
    elif kind == "zero":
        eye[0] = 0.0
        eye[1] = -0.0
    elif kind == "irregular":
        eye[0] = 1e-12                # below 2^-36: every node takes the reference's own divisions
    else:
        eye[2] = eye[2] + 1e-3
        eye[0] = -3e-20
    d = _desc(name, eye)
    _compare(sc, d, 64, 48, 4, tiled=True)
    _compare(sc, d, 40, 30, 1, tiled=False, any_shadow=True)


@pytest.mark.parametrize("name", ["sponza", "bunny"])
def test_eye_inside_and_outside_the_root_box(miro, name):
    sc = product_scene(miro, name)
    lo, hi = _root_box(sc)
    inside = _desc(name, (lo + hi) * np.float32(0.5) + (hi - lo) * np.float32(0.125))
    assert all(lo[k] < inside["eye"][k] < hi[k] for k in range(3))
    _compare(sc, inside, 96, 54, 16, tiled=True)
    outside = _desc(name, (float(hi[0]) + 5.0, float(hi[1]) + 1.0, float(lo[2]) - 2.0))
    _compare(sc, outside, 96, 54, 4, tiled=True)


@pytest.mark.parametrize("name", ["sponza", "cornell"])
def test_any_hit_shadows(miro, name):
    sc = product_scene(miro, name)
    _compare(sc, _desc(name), 80, 45, 4, tiled=True, any_shadow=True)


def test_banded_ranks(miro):
    name, W, H, spp, band, world = "sponza", 96, 54, 4, 6, 3
    sc = product_scene(miro, name)
    d = _desc(name, (6.0, 2.0, 0.5))
    ref = mframe.FrameRenderer(sc, d, W, H, spp=spp)
    ref.generate()
    ref.step()
    full = torch.zeros((H, W, 3), dtype=torch.float32, device="cuda")
    for r in range(world):
        fu = mframe.FusedFrame(sc, d, W, H, spp=spp, band=band, rank=r, world=world)
        fu.step()
        rows = torch.from_numpy(mframe.rows_of(mframe.band_rows(H, band, r, world))).to("cuda")
        full[rows] = fu.d_rgb.view(len(rows), W, 3)
    torch.cuda.synchronize()
    assert np.array_equal(_bits(full.view(-1, 3)), _bits(ref.d_rgb))


def test_no_shadow_rays(miro):
    name, W, H = "teapot", 96, 64
    sc = product_scene(miro, name)
    d = _desc(name, (1.0, 2.5, 5.5))
    ref = mframe.FrameRenderer(sc, d, W, H, spp=1)
    ref.generate()
    ref.step()
    fu = mframe.FusedFrame(sc, d, W, H, spp=1, keep_hits=True, tiled=False, no_shadows=True)
    fu.step()
    torch.cuda.synchronize()
    assert np.array_equal(_bits(fu.d_hits), _bits(ref.d_hits))
    assert fu.ray_counts() == (W * H, 0)


def test_per_object_materials(miro):
    """MAT kernels: the eye-relative primary trace and the shading from the eye in the arguments, against one level of the
    recursion over resident eye rays (mr_trace_level, scene tables) -- one sample per pixel: the same bits"""
    name, W, H = "sponza", 96, 54
    sc = product_scene(miro, name)
    n_tri = int(sc.info().n_triangles)
    sc.set_materials([((0.8, 0.7, 0.6), (0.3, 0.3, 0.3), (0.0, 0.0, 0.0), 12.0, 1.0),
                      ((0.2, 0.5, 0.9), (0.0, 0.0, 0.0), (0.0, 0.0, 0.0), 1.0, 1.0)],
                     (np.arange(n_tri) % 2).astype(np.uint32))
    for eye in (None, (1e-12, 2.0, 0.5)):
        d = _desc(name, eye)
        fu = mframe.FusedFrame(sc, d, W, H, spp=1, keep_hits=True, tiled=False)
        fu.step()
        fr = mframe.FrameRenderer(sc, d, W, H, spp=1)
        fr.generate()
        fr.render_specular(depth=0, fused=True)
        tr = mframe.FrameRenderer(sc, d, W, H, spp=1)
        tr.generate()
        sc.trace_device(tr.d_rays, tr.n, tr.d_hits)
        torch.cuda.synchronize()
        assert np.array_equal(_bits(fu.d_hits), _bits(tr.d_hits))
        assert torch.equal(fr.d_rgb, fu.d_rgb)


def test_overlapping_calls_with_different_cameras(miro):
    """calls in flight on two streams with two cameras -- and the first camera again on the second stream, which takes the
    tables built on the first one: each equals its own render on one stream"""
    name, W, H, spp = "sponza", 128, 72, 16
    sc = product_scene(miro, name)
    da, db = _desc(name), _desc(name, (-6.0, 3.0, 1.5))
    want = []
    for d in (da, db):
        fu = mframe.FusedFrame(sc, d, W, H, spp=spp, keep_hits=True)
        fu.step()
        torch.cuda.synchronize()
        want.append((_bits(fu.d_rgb), _bits(fu.d_hits)))
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    fa = mframe.FusedFrame(sc, da, W, H, spp=spp, keep_hits=True)
    fb = mframe.FusedFrame(sc, db, W, H, spp=spp, keep_hits=True)
    fa2 = mframe.FusedFrame(sc, da, W, H, spp=spp, keep_hits=True)
    torch.cuda.synchronize()
    for k in range(3):
        eye = (-6.0 + k, 3.0, 1.5)
        with torch.cuda.stream(s1):
            mframe.FusedFrame(sc, _desc(name, (1.0 + k, 2.0, 0.0)), 16, 16, spp=1).step(stream=s1)   # new tables on s1
            fa.step(stream=s1)
        with torch.cuda.stream(s2):
            fb.step(stream=s2)
            fa2.step(stream=s2)
        torch.cuda.synchronize()
        for f, w in ((fa, want[0]), (fb, want[1]), (fa2, want[0])):
            assert np.array_equal(_bits(f.d_rgb), w[0]) and np.array_equal(_bits(f.d_hits), w[1]), (k, eye)


def test_cameras_taking_turns(miro):
    """two cameras in turn on one stream, then 70 others (every table set rebuilt), then the first two again"""
    name, W, H, spp = "bunny", 48, 32, 4
    sc = product_scene(miro, name)
    eyes = [None, (3.0, 4.0, 12.0)]
    want = []
    for e in eyes:
        fu = mframe.FusedFrame(sc, _desc(name, e), W, H, spp=spp, keep_hits=True)
        fu.step()
        torch.cuda.synchronize()
        want.append(_bits(fu.d_hits))
    frames = [mframe.FusedFrame(sc, _desc(name, e), W, H, spp=spp, keep_hits=True) for e in eyes]
    for rnd in range(2):
        for _ in range(3):
            for f, w in zip(frames, want):
                f.d_hits.zero_()
                f.step()
                torch.cuda.synchronize()
                assert np.array_equal(_bits(f.d_hits), w), rnd
        for k in range(70):
            mframe.FusedFrame(sc, _desc(name, (0.1 * k, 5.0, 15.0)), 8, 8, spp=1).step()


def test_graph_replay_rebuilds_its_tables(miro):
    """a captured call holds its table build: replayed after 70 calls with other cameras have rebuilt every table set, the
    graph still renders its own camera"""
    name, W, H, spp = "bunny", 64, 48, 4
    sc = product_scene(miro, name)
    d = _desc(name)
    ref = mframe.FusedFrame(sc, d, W, H, spp=spp, keep_hits=True)
    ref.step()
    torch.cuda.synchronize()
    fu = mframe.FusedFrame(sc, d, W, H, spp=spp, keep_hits=True)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        fu.step(stream=side)
    for rep in range(2):
        fu.d_rgb.zero_()
        fu.d_hits.zero_()
        for k in range(70):
            mframe.FusedFrame(sc, _desc(name, (2.0 + 0.1 * k, 4.0, 10.0 + rep)), 8, 8, spp=1).step()
        g.replay()
        torch.cuda.synchronize()
        assert np.array_equal(_bits(fu.d_rgb), _bits(ref.d_rgb)), rep
        assert np.array_equal(_bits(fu.d_hits), _bits(ref.d_hits)), rep
        # and a direct call with the graph's camera afterwards is not confused by the replay
        fu.d_hits.zero_()
        fu.step()
        torch.cuda.synchronize()
        assert np.array_equal(_bits(fu.d_hits), _bits(ref.d_hits)), rep
