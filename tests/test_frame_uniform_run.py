"""The uniform run of the fused frame kernel (mr_traverse.h: uniform_run): once a wave is found at one node, the node index
stays a scalar for as long as every active lane takes the same decision.  Every lane keeps its own stack and the arithmetic of a
visit is untouched, so primary records, shadow records and pixels must be the batched pipeline's (mr_trace ->
mr_gen_shadow_rays -> mr_trace_indirect -> shade, which has no run) and the oracle's, byte for byte.

Windows are 16x8 pixels: at 64 samples per pixel a wave is one pixel (the run starts and continues in interior pixels, splits
and restarts on silhouettes), at 16 spp four pixels, at 1 spp 64 pixels (the run hardly ever starts).

That a case reaches the path it is about is asserted on the CPU (replay_first_descent: each wave's way from the root to its
first leaf, in float32 on the exported tree): runs that continue, runs that split, near-tie visits inside a run, irregular
nodes met inside a run."""
import numpy as np
import pytest
import torch

from helpers import product_scene
from miro_amd import frame as mframe
from miro_amd import scenes

pytestmark = pytest.mark.gpu

# narrow views that put an object's edge across the window
VIEWS = {
    "teapot": dict(lookat=(1.6, 1.0, 0.0), fov=10.0),         # the spout / body edge against the floor triangle
    "cornell": dict(lookat=(1.9, 1.2, -1.6), fov=14.0),       # an edge of a block against the walls behind it
}


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32).numpy()


def _desc(name, **over):
    d = dict(scenes.SCENES[name])
    d.update(VIEWS.get(name, {}))
    d.update(over)
    for k in ("eye", "lookat", "light"):
        d[k] = tuple(float(np.float32(v)) for v in d[k])
    return d


def _oracle_scene(oracle, d):
    s = oracle.Scene()
    scenes.populate(s, d)
    s.build(4)
    return s


def _regular_dir(d):
    ad = np.abs(d)
    return ((ad >= 2.0 ** -40) & (ad <= 2.0 ** 40)).all(axis=1)


def _regular_pos(o):
    ao = np.abs(o)
    return ((ao == 0) | ((ao >= 2.0 ** -36) & (ao <= 2.0 ** 60))).all(axis=1)


def _irregular_box(c):
    a = np.abs(c)
    return bool((~np.isfinite(c) | ((a != 0) & ((a < 2.0 ** -36) | (a > 2.0 ** 60)))).any())


def _pattern_distance(a, b):
    """v_sad_u32 on the bit patterns of two float32 arrays"""
    return np.abs(a.view(np.uint32).astype(np.int64) - b.view(np.uint32).astype(np.int64))


def replay_first_descent(corners, meta, rays):
    """What uniform_run does with each 64-ray wave of eye rays between the root and its first leaf, replayed in float32 on the
    exported tree (node i tests the boxes of its children meta[i, 1:3]; the eye-relative tables hold corner - eye, the same
    subtraction, and an irregular eye marks every node irregular).  Until the first leaf the rays' tMax is still the callers', so the
    visits, the guard's pattern distances and the decisions are exactly the kernel's.  Returns (visits inside runs, visits at
    which some lane had a pair of NON-ZERO values within 16 patterns -- the wave recomputes the node with exact quotients --,
    visits of irregular nodes, runs ended by a split decision).  A near-tie visit is decided like the kernel's, from the correctly
    rounded quotients (float32 division), and the descent goes on; it stops at an irregular node, a split or a pop.  Only the
    primary rays' first descent is replayed: restarts after a pop and the runs of the shadow trace are covered by the
    byte-for-byte comparisons alone."""
    f = np.float32
    o = np.stack([rays["ox"], rays["oy"], rays["oz"]], 1).astype(f)
    d = np.stack([rays["dx"], rays["dy"], rays["dz"]], 1).astype(f)
    tmax = rays["tmax"].astype(f)
    visits = ties = irregular = splits = 0
    with np.errstate(all="ignore"):
        inv = f(1.0) / d
        for w in range(len(rays) // 64):
            sl = slice(64 * w, 64 * w + 64)
            ow, dw, iw, tw = o[sl], d[sl], inv[sl], tmax[sl]
            neg = dw < 0
            if not (neg == neg[0]).all() or not _regular_dir(dw).all() or (rays["tmin"][sl] != 0).any():
                continue                                     # no octant loop for this wave

            def slabs(box, exact=False):
                near = np.where(neg[0], box[3:], box[:3]).astype(f)
                far = np.where(neg[0], box[:3], box[3:]).astype(f)
                if exact:
                    return ((near - ow) / dw).max(axis=1), ((far - ow) / dw).min(axis=1)
                return ((near - ow) * iw).max(axis=1), ((far - ow) * iw).min(axis=1)

            mn, mx = slabs(corners[0])
            act = ~((mn > mx) | (mn > tw) | (mx < 0))
            if not act.any() or meta[0, 0]:
                continue
            cur = 0
            while not meta[cur, 0]:
                c0, c1 = int(meta[cur, 1]), int(meta[cur, 2])
                visits += 1
                if not _regular_pos(ow).all() or _irregular_box(corners[c0]) or _irregular_box(corners[c1]):
                    irregular += 1
                    break
                mn0, mx0 = slabs(corners[c0])
                mn1, mx1 = slabs(corners[c1])
                k0, k1 = np.minimum(mx0, tw), np.minimum(mx1, tw)
                close = np.zeros(64, bool)
                for a, b in ((mn0, k0), (mn1, k1), (mn0, mn1)):
                    close |= (_pattern_distance(a, b) <= 16) & (a != 0) & (b != 0)
                if (close & act).any():
                    ties += 1
                    mn0, mx0 = slabs(corners[c0], exact=True)
                    mn1, mx1 = slabs(corners[c1], exact=True)
                    k0, k1 = np.minimum(mx0, tw), np.minimum(mx1, tw)
                h0 = ~((mn0 > k0) | (mx0 < 0))
                h1 = ~((mn1 > k1) | (mx1 < 0))
                first1 = mn0 > mn1
                if (h0 & h1)[act].all() and (first1[act].all() or not first1[act].any()):
                    cur = c1 if first1[act].all() else c0
                elif h0[act].all() and not h1[act].any():
                    cur = c0
                elif h1[act].all() and not h0[act].any():
                    cur = c1
                else:
                    if (h0 | h1)[act].any():
                        splits += 1
                    break
    return visits, ties, irregular, splits


def _check(miro, oracle, d, W, H, spp, sc=None):
    """fused frame against the batched pipeline and against the oracle on the batched pipeline's rays"""
    if sc is None:
        sc = miro.Scene(0)
        scenes.populate(sc, d)
        sc.build(4)
    ref = mframe.FrameRenderer(sc, d, W, H, spp=spp, tiled=False)
    ref.generate()
    ref.step()
    fu = mframe.FusedFrame(sc, d, W, H, spp=spp, tiled=False, keep_hits=True)
    fu.step()
    torch.cuda.synchronize()
    n_p, n_s = ref.ray_counts()
    assert fu.ray_counts() == (n_p, n_s)
    assert np.array_equal(_bits(fu.d_hits), _bits(ref.d_hits))
    src = ref.d_src[:n_s].to(torch.int64)
    assert np.array_equal(_bits(fu.d_shadow_hits[src]), _bits(ref.d_shadow_hits[:n_s]))
    assert np.array_equal(_bits(fu.d_rgb), _bits(ref.d_rgb))
    osc = _oracle_scene(oracle, d)
    rays = np.frombuffer(ref.d_rays.cpu().numpy().tobytes(), dtype=oracle.RAY_DTYPE)
    want = osc.trace(rays)
    assert fu.d_hits.cpu().numpy().tobytes() == want.tobytes(), "primary records differ from the oracle"
    if n_s:
        srays = np.frombuffer(ref.d_shadow_rays[:n_s].cpu().numpy().tobytes(), dtype=oracle.RAY_DTYPE)
        want_s = osc.trace(srays)
        assert fu.d_shadow_hits[src].cpu().numpy().tobytes() == want_s.tobytes(), "shadow records differ from the oracle"
    prim = fu.d_hits.cpu().numpy().view(miro.HIT_DTYPE).reshape(-1)["prim"]
    corners, meta, _ = sc.export_tree()
    replay = replay_first_descent(corners, meta, rays) if spp == 64 else None
    shadow = (ref.d_shadow_rays[:n_s].cpu().numpy(), src.cpu().numpy())
    return prim, replay, shadow


@pytest.mark.parametrize("name", ["teapot", "cornell"])
@pytest.mark.parametrize("spp", [64, 16, 1])
def test_window(miro, oracle, name, spp):
    prim, replay, _ = _check(miro, oracle, _desc(name), 16, 8, spp)
    if spp == 64:       # the window holds pixels whose samples part (silhouette) and pixels whose samples see one triangle
        per_pixel = [len(set(p.tolist())) for p in prim.reshape(-1, 64)]
        assert max(per_pixel) > 1 and min(per_pixel) == 1, per_pixel
        visits, ties, irregular, splits = replay
        # runs start, some go on beyond their first visit, some end on a split decision
        assert visits > 16 * 8 and splits >= 1 and irregular == 0, replay


def test_ragged_last_wave(miro, oracle):
    # 13 x 7 pixels x 16 samples = 1 456 samples: the last chunk is ragged and its last wave has 48 live lanes
    _check(miro, oracle, _desc("teapot"), 13, 7, 16)


def _slab_eye(sc, eye):
    corners, _, _ = sc.export_tree()
    fin = corners[np.isfinite(corners).all(axis=1)]
    e = list(np.float32(eye))
    for k in (0, 1):
        vals = np.concatenate([fin[:, k], fin[:, 3 + k]])
        e[k] = vals[np.argmin(np.abs(vals - e[k]))]
    return e


@pytest.mark.parametrize("kind", ["slab", "irregular"])
def test_special_eyes(miro, oracle, kind):
    sc = product_scene(miro, "teapot")
    eye = list(scenes.SCENES["teapot"]["eye"])
    if kind == "slab":
        eye = _slab_eye(sc, eye)         # relative corners of exactly 0 on two axes, the root box's planes among them
    else:
        eye[0] = 1e-12                   # below 2^-36: every node is irregular, every visit leaves the run for the true divisions
    _, replay, _ = _check(miro, oracle, _desc("teapot", eye=eye), 16, 8, 64, sc=sc)
    if kind == "irregular":
        assert replay[2] >= 1 and replay[0] == replay[2], replay     # every run's first visit is an irregular one
    else:
        assert replay[0] >= 1, replay


def test_shadow_rays_straddle_octants(miro, oracle):
    # the light straight above the patch of floor in view: a pixel's shadow rays have dx and dz of both signs, so the wave
    # takes the generic loop (no run) for them
    d = _desc("teapot", lookat=(3.0, 0.0, 0.0), fov=6.0, light=(3.0, 10.0, 0.0))
    _, _, (srays, src) = _check(miro, oracle, d, 16, 8, 64)
    straddling = 0
    for pixel in np.unique(src // 64):
        dirs = srays[src // 64 == pixel][:, 4:7]
        straddling += int(((dirs < 0).any(axis=0) & (dirs > 0).any(axis=0)).any())
    assert straddling >= 1, "no pixel whose shadow rays point into two octants"


def test_irregular_node_reached_by_uniform_waves(miro, oracle):
    # a triangle with corners beyond 2^60: its box and every box around it, a child of the root among them, are irregular --
    # each wave meets them at the top of the tree, uniform, from inside a run and has to divide
    huge = ("triangle", (-2e18, -0.5, -2e18, 0.0, -0.5, 2e18, 2e18, -0.5, -2e18), (0, 1, 0) * 3)
    d = _desc("teapot", objects=[huge])
    _, replay, _ = _check(miro, oracle, d, 16, 8, 64)
    assert replay[2] >= 1, replay


def test_grazing_wall(miro, oracle):
    # a wall of the Cornell box seen at grazing incidence: slab-distance ties cluster there, which is
    # where the guard falls back to exact quotients.  On the CPU this camera gives 64 waves whose first visit -- inside a run
    # -- has two non-zero values within 16 patterns (the root's children share the face the rays enter through).
    d = _desc("cornell", eye=(0.02, 2.5, 3.0), lookat=(0.0, 2.5, -2.0), fov=20.0)
    _, replay, _ = _check(miro, oracle, d, 16, 8, 64)
    assert replay[1] >= 1, replay
