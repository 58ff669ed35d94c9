"""The scalar side of a wave-uniform visit in the fused frame kernel (mr_traverse.h: uniform_run): the run keeps its node as a
byte offset for the scalar load, leaves through values of the node reference that are no reference (kDone, kRunIrregular) instead
of a lane mask, and takes its decision from the compare masks as they are.  No floating-point instruction, operand or order of
a lane's steps changes, so primary records, shadow records and pixels of FusedFrame(keep_hits=True) must be FrameRenderer's --
the batched kernels take no run -- bit for bit (the comparison of test_fused_frame.py's _compare).

That a case reaches the path it is about is asserted on the CPU: split decisions through test_frame_uniform_run.py's replay of
each wave's first descent, leaf shapes and the last record of the triangle table from the exported tree and the hit records
(the uniform leaf loop of these walks is the one before; the scene stays as the check of whatever is done to it next)."""
import numpy as np
import pytest
import torch

from helpers import product_scene
from miro_amd import frame as mframe
from miro_amd import scenes
from test_frame_uniform_run import replay_first_descent

pytestmark = pytest.mark.gpu


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32).numpy()


def _desc(name, **over):
    d = dict(scenes.SCENES[name])
    d.update(over)
    for k in ("eye", "lookat", "light"):
        d[k] = tuple(float(np.float32(v)) for v in d[k])
    return d


def _scene_of(miro, d):
    sc = miro.Scene(0)
    scenes.populate(sc, d)
    sc.build(4)
    return sc


def _compare(sc, d, W, H, spp, tiled, any_shadow=False, no_shadows=False):
    """primary records, shadow records, ray counts and pixels of the fused frame against the batched pipeline, raw bits"""
    ref = mframe.FrameRenderer(sc, d, W, H, spp=spp, tiled=tiled)
    ref.generate()
    if no_shadows:                       # the reference's -DDISABLE_SHADOWS build: no shadow ray is traced, every hit is lit --
        ref.trace_primary()              # the batched shade given a miss record for every shadow ray it made
        ref.make_shadow_rays()
        ref.d_shadow_hits.zero_()
        ref.d_shadow_hits.view(torch.int32)[:, 1] = -1
        ref.shade()
    else:
        ref.step(any_hit=any_shadow)
    fu = mframe.FusedFrame(sc, d, W, H, spp=spp, tiled=tiled, keep_hits=True, any_shadow=any_shadow, no_shadows=no_shadows)
    fu.step()
    torch.cuda.synchronize()
    assert np.array_equal(_bits(fu.d_hits), _bits(ref.d_hits))
    if no_shadows:
        assert fu.ray_counts() == (ref.n, 0)
        assert (fu.d_shadow_hits[:, 0] == 0).all() and (fu.d_shadow_hits[:, 1].view(torch.int32) == -1).all()
        n_s, src = 0, None
    else:
        n_p, n_s = ref.ray_counts()
        assert fu.ray_counts() == (n_p, n_s)
        src = ref.d_src[:n_s].to(torch.int64)
        assert np.array_equal(_bits(fu.d_shadow_hits[src]), _bits(ref.d_shadow_hits[:n_s]))
        no_ray = torch.ones(ref.n, dtype=torch.bool, device=src.device)
        no_ray[src] = False
        rest = fu.d_shadow_hits[no_ray]
        assert (rest[:, 0] == 0).all() and (rest[:, 1].view(torch.int32) == -1).all()
    assert np.array_equal(_bits(fu.d_rgb), _bits(ref.d_rgb))
    return fu, ref, n_s, src


def _replay(miro, oracle, sc, ref):
    rays = np.frombuffer(ref.d_rays.cpu().numpy().tobytes(), dtype=oracle.RAY_DTYPE)
    corners, meta, _ = sc.export_tree()
    return replay_first_descent(corners, meta, rays)


def test_long_runs_one_pixel_per_wave(miro, oracle):
    # the stand-in atrium, 32 x 18 at 64 samples per pixel in image order: a wave is one pixel, runs are long (the 128-lane build)
    sc = product_scene(miro, "sponza")
    _, ref, n_s, _ = _compare(sc, _desc("sponza"), 32, 18, 64, False)
    visits, _, irregular, _ = _replay(miro, oracle, sc, ref)
    assert n_s > 0 and irregular == 0 and visits > 4 * 32 * 18, visits       # runs go on beyond their first visits


@pytest.mark.parametrize("spp,tiled", [(4, True), (1, True)])
def test_waves_straddle_pixels(miro, oracle, spp, tiled):
    # 64 x 36 in the tiled order: a wave is a tile of 4 x 4 or 8 x 8 pixels, so runs end on splits and pops and L.cur, the stack and
    # the pushed reference are handed over lane by lane
    sc = product_scene(miro, "sponza")
    _, ref, n_s, _ = _compare(sc, _desc("sponza"), 64, 36, spp, tiled)
    visits, _, _, splits = _replay(miro, oracle, sc, ref)
    assert n_s > 0 and visits >= 1 and splits >= 1, (visits, splits)         # at least one run ended on a split decision


def test_irregular_eye(miro, oracle):
    # one eye component below 2^-36: every node of the eye-relative table is irregular, every visit leaves the run through
    # kRunIrregular
    sc = product_scene(miro, "teapot")
    eye = list(scenes.SCENES["teapot"]["eye"])
    eye[0] = 1e-12
    d = _desc("teapot", eye=eye, lookat=(1.6, 1.0, 0.0), fov=10.0)
    _, ref, _, _ = _compare(sc, d, 16, 8, 64, False)
    visits, _, irregular, _ = _replay(miro, oracle, sc, ref)
    assert irregular >= 1 and visits == irregular, (visits, irregular)


def test_irregular_node_mid_run(miro, oracle):
    # a triangle with corners beyond 2^60: its box and every box around it are irregular and are met from inside a run
    huge = ("triangle", (-2e18, -0.5, -2e18, 0.0, -0.5, 2e18, 2e18, -0.5, -2e18), (0, 1, 0) * 3)
    d = _desc("teapot", objects=[huge], lookat=(1.6, 1.0, 0.0), fov=10.0)
    sc = _scene_of(miro, d)
    _, ref, _, _ = _compare(sc, d, 16, 8, 64, False)
    assert _replay(miro, oracle, sc, ref)[2] >= 1


# ---- leaf shapes -----------------------------------------------------------------------------------------------------------
# A row of square cards along x, tilted 45 degrees about y so that the camera (in front, +z) sees every one of them and a shadow
# ray towards the light (far out on +x) from one card meets the next.  Card k is cut into CARDS[k] triangles (a fan around one
# corner: they share no box), or is 16 times the same triangle -- a leaf the builder cannot split, so its count is extended.
CARDS = (4, 1, 4, 2, 4, 3, 16, 4, 2, 16, 1, 4)


def _card(cx, n):
    h = 0.5
    s = np.float32(np.sqrt(0.5))

    def at(u, v):                        # card coordinates -> world: u runs along (1, 0, -1) / sqrt 2, v along y
        return (float(cx + u * h * s), float(v * h), float(-u * h * s))
    nrm = (float(s), 0.0, float(s)) * 3
    if n == 16:
        tri = at(-1, -1) + at(1, -1) + at(0, 1)
        return [("triangle", tri, nrm)] * 16
    if n == 1:
        return [("triangle", at(-1, -1) + at(1, -1) + at(0, 1), nrm)]
    # a fan around the corner (-1, -1) over n + 1 points along the two far edges of the square
    t = np.linspace(0.0, 2.0, n + 1)
    rim = [(1.0, min(1.0, -1.0 + 2.0 * x)) if x <= 1.0 else (1.0 - 2.0 * (x - 1.0), 1.0) for x in t]
    return [("triangle", at(-1, -1) + at(*rim[i]) + at(*rim[i + 1]), nrm) for i in range(n)]


def leaf_shape_desc():
    objs = []
    for k, n in enumerate(CARDS):
        objs += _card(1.5 * k, n)
    span = 1.5 * (len(CARDS) - 1)
    return dict(models=[], floor=None, objects=objs, eye=(span / 2, 0.0, 9.0), lookat=(span / 2, 0.0, 0.0), up=scenes.UP, fov=15.0,
                light=(span + 40.0, 0.0, 0.0), wattage=4000.0)


def _leaf_counts(sc):
    _, meta, prims = sc.export_tree()
    leaves = meta[meta[:, 0] != 0]
    return leaves[:, 1], leaves[:, 2], prims


@pytest.mark.parametrize("spp,W,H", [(64, 48, 6), (4, 96, 12)])
def test_leaf_shapes_and_the_last_record(miro, spp, W, H):
    d = leaf_shape_desc()
    d = _desc_of(d)
    sc = _scene_of(miro, d)
    first, count, prims = _leaf_counts(sc)
    assert {1, 2, 3, 4} <= set(count.tolist()) and count.max() >= 15, sorted(set(count.tolist()))
    assert int((first + count).max()) == len(prims)                       # the last leaf ends at the table's end
    last = int(prims[-1])                                                  # the object whose record is the table's last
    fu, ref, n_s, src = _compare(sc, d, W, H, spp, spp < 64)
    prim = fu.d_hits.cpu().numpy().view(miro.HIT_DTYPE).reshape(-1)["prim"]
    sprim = fu.d_shadow_hits[src].cpu().numpy().view(miro.HIT_DTYPE).reshape(-1)["prim"]
    assert (prim == last).any(), "no camera ray reports the last record"
    assert (sprim == last).any(), "no shadow ray reports the last record"
    big = np.nonzero(count >= 15)[0]                                       # ... and the extended-count leaves are hit by both
    in_big = np.concatenate([prims[first[i]:first[i] + count[i]] for i in big])
    assert np.isin(prim, in_big).any() and np.isin(sprim, in_big).any()


def _desc_of(d):
    d = dict(d)
    for k in ("eye", "lookat", "light"):
        d[k] = tuple(float(np.float32(v)) for v in d[k])
    return d


@pytest.mark.parametrize("mode", ["any_shadow", "no_shadows"])
def test_shadow_forms(miro, mode):
    # any-hit shadow rays and the launch without shadow rays: the SHADOW forms of the kernel share the loops
    sc = product_scene(miro, "sponza")
    _compare(sc, _desc("sponza"), 48, 27, 16, True, any_shadow=mode == "any_shadow", no_shadows=mode == "no_shadows")


def test_per_object_materials_take_no_run(miro):
    # A scene with a material table is shaded per object (the MAT kernels): kRun is false there and the walk is the one before.
    # The batched shade refuses such a scene, so the records are compared with the batched traces and the picture with one level
    # of the recursion (mr_trace_level) at one sample per pixel, where no summation order can differ.
    d = _desc("cornell")
    sc = miro.Scene(0)
    n = scenes.populate(sc, d)
    mats = [((0.8, 0.2, 0.2), (0, 0, 0), (0, 0, 0), 1.0, 1.0), ((0.2, 0.8, 0.3), (0, 0, 0), (0, 0, 0), 1.0, 1.0)]
    sc.set_materials(mats, (np.arange(n) % 2).astype(np.uint32))
    sc.build(4)
    for W, H, spp in ((33, 31, 64), (66, 62, 1)):
        ref = mframe.FrameRenderer(sc, d, W, H, spp=spp, tiled=False)
        ref.generate()
        ref.trace_primary()
        ref.make_shadow_rays()
        ref.trace_shadow()
        fu = mframe.FusedFrame(sc, d, W, H, spp=spp, tiled=False, keep_hits=True)
        fu.step()
        torch.cuda.synchronize()
        n_s = int(ref.d_count.item())
        assert fu.ray_counts() == (ref.n, n_s) and n_s > 0
        assert np.array_equal(_bits(fu.d_hits), _bits(ref.d_hits))
        src = ref.d_src[:n_s].to(torch.int64)
        assert np.array_equal(_bits(fu.d_shadow_hits[src]), _bits(ref.d_shadow_hits[:n_s]))
        if spp == 1:
            ref.render_specular(depth=0, fused=True)
            torch.cuda.synchronize()
            assert float(fu.d_rgb.max()) > 0 and np.array_equal(_bits(fu.d_rgb), _bits(ref.d_rgb))
