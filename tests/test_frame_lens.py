"""mr_render_level_lights_lens on the MI355X (csrc/mr_frame_lens.hip, include/miro_hip_lens.h): the level-0 frame of
mr_render_level_lights whose eye rays go through the thin lens (Camera::eyeRay under -DDOF, Camera.cpp:135-160, Miro.h:18-19).

The yardstick is the batched route the parent commit renders a depth-of-field frame with: lens_queue() makes
mr_gen_eye_rays_lens' rays for the window, range by range in the frame's order, and mr_trace_level_lights (MR_LEVEL_SPECULAR) /
mr_trace_level_lights_path (MR_LEVEL_PATH, the same kinds and seed, bounce 0) run on that queue with weights and ids NULL and
d_pixels = the window pixel of every sample.  Against it, bit for bit: hit records, per-sample colour, normal and radiance, the
five counters, d_out_count and the children (specular: sorted record sets; path: by child id, with octant and low-res byte).
The pixels are compared against a numpy fp32 restatement of the body's butterfly over the per-sample radiance that was just
proven equal: for off = 1, 2, 4, ... < spp: L = L + L[k ^ off]; lane sm == 0; x float32(1) / float32(spp); NaN by position.
Every yardstick first shows on its own side that the case is not empty (hits, misses in an open scene, light, children) and
that its rays differ from the pinhole generator's for the same seed.

Which case launches which of the eighteen frame kernels (variant x CHILDREN 0 / 1 / 2 = MR_LEVEL_LAST / SPECULAR / PATH):
  kTraceExact        0, 1, 2   test_shapes_where_it_can_go_wrong (textured teapot, no flags), test_apertures, the flower
  kTraceProduct      0, 1, 2   test_flag_cases_on_the_teapot (MR_MATH_PRODUCT)
  kTraceVote         0, 1, 2   test_flag_cases_on_the_teapot (MR_TRACE_INCOHERENT)
  kTraceVoteProduct  0, 1, 2   test_flag_cases_on_the_teapot (both)
  kTraceExactObj     0, 1, 2   test_mixed_room (no flags, and MR_TRACE_INCOHERENT, which a scene with objects ignores); 1, 2 also
                               the stone room and the glass sphere
  kTraceProductObj   0, 1, 2   test_mixed_room (MR_MATH_PRODUCT, and both flags)"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_frame_level_lights import (COUNTS0, GLASS_DESC, PATH, SPECULAR, Level0, assert_path_children, assert_spec_children, cuda,  # noqa: E402
                                     path_kinds_of, window_ranges)
from test_frame_lights import MISS, SENTINEL, bits, camera, same  # noqa: E402
from test_level_lights import ENVS, use  # noqa: E402
from test_level_lights import Fused as SpecLevel  # noqa: E402
from test_level_lights_path import BYTE, ID, PIX, Q, child_id, glass_sphere  # noqa: E402
from test_level_lights_path import Fused as PathLevel  # noqa: E402

F = np.float32
LAST = 0
APERTURE = 0.2


def focus_of(desc):
    """a focus plane near the scene's eye-to-lookat distance"""
    return float(np.linalg.norm(np.asarray(desc["lookat"], dtype=np.float64) - np.asarray(desc["eye"], dtype=np.float64)))


class LensScene:
    """the scene as Level0 (tests/test_frame_level_lights.py) drives it, with render_level_lights going through the lens"""

    def __init__(self, scene, aperture, focus_plane):
        self.scene, self.aperture, self.focus_plane = scene, aperture, focus_plane

    def render_level_lights(self, cam, W, H, d_rgb, **kw):
        return self.scene.render_level_lights_lens(cam, W, H, d_rgb, self.aperture, self.focus_plane, **kw)


def level0(miro, scene, desc, W, H, spp, children, env, aperture=APERTURE, focus=None, **kw):
    focus = focus_of(desc) if focus is None else focus
    return Level0(miro, LensScene(scene, aperture, focus), desc, W, H, spp, False, children, env, **kw)


def lens_queue(miro, scene, desc, W, H, spp, aperture=APERTURE, focus=None, y0=0, y1=None, bands=None):
    """the queue mr_gen_eye_rays_lens makes for the window, range by range in the frame's order, and the window pixel of every
    sample: (rays, pixels, n).  With an open lens the rays are not the pinhole generator's."""
    import torch
    focus = focus_of(desc) if focus is None else focus
    ranges = window_ranges(miro, H, y0, y1, bands)
    n = sum(b - a for a, b in ranges) * W * spp
    rays = torch.empty((max(n, 1), 8), dtype=torch.float32, device="cuda")
    pinhole = torch.empty_like(rays)
    pix, off = [], 0
    for a, b in ranges:
        k = (b - a) * W * spp
        scene.gen_eye_rays_lens(camera(desc), W, H, rays[off:off + k], aperture, focus, y0=a, y1=b, spp=spp, jitter=spp > 1, seed=168)
        scene.gen_eye_rays(camera(desc), W, H, pinhole[off:off + k], y0=a, y1=b, spp=spp, jitter=spp > 1, seed=168)
        pix.append(np.arange(k, dtype=np.int64) // spp + off // spp)
        off += k
    torch.cuda.synchronize()
    if n and aperture > 0:
        moved = (rays[:n, :3] != pinhole[:n, :3]).any(dim=1)
        assert float(moved.float().mean()) > 0.9 and not same(rays[:n, 4:7], pinhole[:n, 4:7])
    if n and aperture == 0:
        assert same(rays[:n, :3], pinhole[:n, :3])                                  # the eye itself
    return rays, cuda(np.concatenate(pix).astype(np.int32)) if n else None, n


def spec_level(miro, scene, desc, W, H, spp, env, flags=0, **lens_window):
    rays, pixels, n = lens_queue(miro, scene, desc, W, H, spp, **lens_window)
    return SpecLevel(scene, rays, None, pixels, n, spp, flags, env, True, n // spp)


def path_level(miro, scene, desc, W, H, spp, env, kinds, flags=0, path_seed=168, **lens_window):
    rays, pixels, n = lens_queue(miro, scene, desc, W, H, spp, **lens_window)
    return PathLevel(scene, Q(rays, None, pixels, None, None, n), spp, flags, env, n // spp, kinds=kinds, seed=path_seed, bounce=0)


def butterfly(L, spp):
    """[pixels, spp, 3] float32 -> [pixels, 3]: the body's butterfly as lane sm == 0 ends it"""
    L = np.ascontiguousarray(L, dtype=F)
    lane, off = np.arange(spp), 1
    while off < spp:
        L = (L + L[:, lane ^ off]).astype(F)
        off <<= 1
    out = L[:, 0]
    return (out * (F(1) / F(spp))).astype(F) if spp > 1 else out


def assert_frame_half(fu, lv, spp, open_scene=True, lit=True):
    """every output of the frame half against the level yardstick on the lens queue, bit for bit, and the pixels against the
    butterfly of the per-sample radiance; the yardstick has hits, misses in an open scene, and light"""
    n = lv.n
    hit = bits(lv.hits[:n])[:, 1] != MISS
    n_hits = int(hit.sum())
    assert n_hits > 0 and (not open_scene or n_hits < n)
    assert lv.counted[0] == n and lv.counted[3] == n - n_hits and lv.counted[1] > 0
    assert fu.n == n and fu.n_pixels * spp == n
    assert np.array_equal(bits(fu.hits[:n]), bits(lv.hits[:n]))
    h = cuda(hit)
    for mine, theirs in ((fu.color, lv.color), (fu.normal, lv.normal)):
        assert same(mine[:n][h], theirs[:n][h])
        assert bool((mine[:n][~h] == SENTINEL).all())                               # a miss keeps what the buffer held
    assert same(fu.sample_rgb[:n], lv.ray_rgb[:n])
    assert fu.counted == lv.counted, (fu.counted, lv.counted)
    want = butterfly(fu.sample_rgb[:n].cpu().numpy().reshape(fu.n_pixels, spp, 3), spp)
    assert not lit or float(np.nanmax(want)) > 0
    assert np.array_equal(fu.rgb[:fu.n_pixels].cpu().numpy(), want, equal_nan=True)


def check_case(miro, scene, desc, W, H, spp, env, kinds=7, path_seed=168, flags=0, open_scene=True, lit=True, last=True, **lens_window):
    """both kinds of children and (last) MR_LEVEL_LAST of one shape against the two level yardsticks; returns (specular level, path
    level, the path frame)"""
    e = ENVS[env]
    sp = spec_level(miro, scene, desc, W, H, spp, e, flags=flags, **lens_window)
    lv = path_level(miro, scene, desc, W, H, spp, e, kinds, flags=flags, path_seed=path_seed, **lens_window)
    fs = level0(miro, scene, desc, W, H, spp, SPECULAR, env, flags=flags, **lens_window)
    assert_frame_half(fs, sp, spp, open_scene, lit)
    assert_spec_children(fs, sp)
    fp = level0(miro, scene, desc, W, H, spp, PATH, env, flags=flags, kinds=kinds, path_seed=path_seed, **lens_window)
    assert_frame_half(fp, lv, spp, open_scene, lit)
    assert_path_children(fp, lv)
    if last:
        fl = level0(miro, scene, desc, W, H, spp, LAST, env, flags=flags, **lens_window)
        assert_frame_half(fl, sp, spp, open_scene, lit)
        assert int(fl.count.item()) == 12345 and fl.untouched(0)                    # the queue arguments are ignored
    return sp, lv, fp


# ---- on the MI355X -------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_shapes_where_it_can_go_wrong(miro):
    """On the textured teapot under the image, both kinds of children and MR_LEVEL_LAST at
      37 x 13 x 1   481 samples: a partial last workgroup, whose lanes past the end are neither misses nor parents;
      rows [9, 21) of 48 x 32 x 2   a window inside the image: the sample key uses the image row;
      bands of 5 rows, rank 1 of 3, of 48 x 32 x 2   rows 5-9 and 20-24, in band order;
      8 x 4 x 64    one pixel per wave, 64 lens origins inside one pixel, the butterfly at full width;
    and an empty window: MR_OK, d_out_count zeroed, nothing else written."""
    scene, desc, lights = use(miro, "teapot_textured", "image")
    cases = [(37, 13, 1, {}), (48, 32, 2, dict(y0=9, y1=21)), (48, 32, 2, dict(bands=(5, 1, 3))), (8, 4, 64, {})]
    for W, H, spp, window in cases:
        sp, lv, fp = check_case(miro, scene, desc, W, H, spp, "image", kinds=3, open_scene=not window, **window)
        assert path_kinds_of(lv)[0] > 0
        top = int(sp.children()[2].max().item())
        assert top < fp.n_pixels and (not window or top >= fp.n_pixels // 2)         # window pixels, up to the window's end
    for children in (SPECULAR, PATH):
        empty = level0(miro, scene, desc, 48, 32, 2, children, "image", y0=7, y1=7, slots=8)
        assert empty.n == 0 and empty.n_children == 0 and empty.counted == (0, 0, 0, 0, 0) and empty.untouched(0)
        for t in (empty.rgb, empty.hits, empty.sample_rgb, empty.color, empty.normal):
            assert bool((t == SENTINEL).all())
    use(miro, "teapot_textured", None)


@pytest.mark.gpu
@pytest.mark.parametrize("aperture", [0.0, 1.0])
def test_apertures(miro, aperture):
    """48 x 32 x 2 on the textured teapot under the image with aperture 0 -- a pinhole through the lens arithmetic: every origin is
    the eye -- and with aperture 1.0, five times the flower scene's"""
    scene, desc, lights = use(miro, "teapot_textured", "image")
    check_case(miro, scene, desc, 48, 32, 2, "image", kinds=3, aperture=aperture)
    use(miro, "teapot_textured", None)


@pytest.mark.gpu
@pytest.mark.parametrize("flags", ["MR_MATH_PRODUCT", "MR_TRACE_INCOHERENT", "both"])
def test_flag_cases_on_the_teapot(miro, flags):
    """48 x 32 x 1 on the textured teapot under the image: the guarded products, the voting traversal, and both"""
    from miro_amd import binding
    f = {"MR_MATH_PRODUCT": binding.MR_MATH_PRODUCT, "MR_TRACE_INCOHERENT": binding.MR_TRACE_INCOHERENT,
         "both": binding.MR_MATH_PRODUCT | binding.MR_TRACE_INCOHERENT}[flags]
    scene, desc, lights = use(miro, "teapot_textured", "image")
    check_case(miro, scene, desc, 48, 32, 1, "image", kinds=3, flags=f)
    use(miro, "teapot_textured", None)


@pytest.mark.gpu
def test_flower_with_drops_under_an_image(miro):
    """flower_scene(drops=True) under the image at 48 x 32 x 2, path_kinds 7: refract, Fresnel and diffuse children, whose low-res
    byte is 1 exactly on the diffuse ones"""
    scene, desc, lights = use(miro, "flower_drops", "image")
    sp, lv, fp = check_case(miro, scene, desc, 48, 32, 2, "image", kinds=7)
    per = path_kinds_of(lv)
    assert per[2] > 0 and per[3] > 0, per
    ids, low = fp.low_by_id()
    hit = np.nonzero(bits(fp.hits[:fp.n])[:, 1] != MISS)[0].astype(np.uint32)
    assert np.array_equal(low == 1, np.isin(ids, child_id(hit, 3))) and 0 < int(low.sum()) < len(low)
    use(miro, "flower_drops", None)


@pytest.mark.gpu
@pytest.mark.parametrize("flags", [0, "MR_MATH_PRODUCT", "MR_TRACE_INCOHERENT", "both"])
def test_mixed_room(miro, flags):
    """The closed room with glass and mirror spheres, a glossy checker plane and five texture kinds, 64 x 32 x 1, path_kinds 7 under
    path seed 29, and the specular children: spheres and planes take the Obj variants, whose hit point starts from the sample's
    own point on the lens"""
    from miro_amd import binding
    f = {0: 0, "MR_MATH_PRODUCT": binding.MR_MATH_PRODUCT, "MR_TRACE_INCOHERENT": binding.MR_TRACE_INCOHERENT,
         "both": binding.MR_MATH_PRODUCT | binding.MR_TRACE_INCOHERENT}[flags]
    scene, desc, lights = use(miro, "mixed", None)
    sp, lv, fp = check_case(miro, scene, desc, 64, 32, 1, None, kinds=7, path_seed=29, flags=f, open_scene=False)
    per = path_kinds_of(lv)
    assert all(p > 0 for p in per) and sum(per) == lv.n_children, per


@pytest.mark.gpu
def test_stone_room(miro):
    """The stone room (closed: every ray hits) at 48 x 32 x 1: the bumped normal and the noise lookups take a hit point that comes
    from the lens origin"""
    scene, desc, lights = use(miro, "stone", None)
    sp, lv, fp = check_case(miro, scene, desc, 48, 32, 1, None, kinds=7, open_scene=False, last=False)
    per = path_kinds_of(lv)
    assert per[3] > 48 * 32 // 8 and per[0] > 0, per


@pytest.mark.gpu
def test_fresnel_children_on_a_glass_sphere(miro):
    """The glass sphere seen from outside at 64 x 48 x 1: parents with two and with three children both occur"""
    s = glass_sphere(miro)
    W, H = 64, 48
    sp, lv, fp = check_case(miro, s, GLASS_DESC, W, H, 1, None, kinds=7, lit=False, last=False)
    per_parent = np.bincount(np.bincount(sp.children()[2].cpu().numpy(), minlength=W * H))
    assert len(per_parent) == 4 and per_parent[1] == 0 and per_parent[2] > 20 and per_parent[3] > 20, per_parent


@pytest.mark.gpu
def test_replays_from_a_captured_graph(miro):
    """After one warm call outside the capture the 48 x 32 x 2 lens frame of the mixed room under the image, with path children, is
    captured into a torch.cuda.graph on one stream and replayed twice, every output refilled with sentinels and d_out_count with a
    wrong value before each replay: the frame half and the child set equal the yardstick's each time."""
    import torch
    scene, desc, lights = use(miro, "mixed", "image")
    W, H, spp = 48, 32, 2
    lv = path_level(miro, scene, desc, W, H, spp, ENVS["image"], 7)
    fu = level0(miro, scene, desc, W, H, spp, PATH, "image")                          # the warm call, a direct launch
    assert_frame_half(fu, lv, spp, open_scene=False)
    assert_path_children(fu, lv)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        fu.launch(torch.cuda.current_stream())
    for _ in range(2):
        for t in (fu.rgb, fu.hits, fu.sample_rgb, fu.color, fu.normal, fu.out[0], fu.out[1]):
            t.fill_(SENTINEL)
        fu.out[2].fill_(PIX)
        fu.out[3].fill_(ID)
        fu.out[4].fill_(BYTE)
        fu.out_low.fill_(BYTE)
        fu.count.fill_(999999)
        fu.counts.copy_(torch.tensor(COUNTS0 + (4242,), dtype=torch.int64))
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        fu.read()
        assert_frame_half(fu, lv, spp, open_scene=False)
        assert_path_children(fu, lv)
    use(miro, "mixed", None)
