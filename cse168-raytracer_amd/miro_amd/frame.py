"""Wavefront frame driver over the C ABI: eye rays -> mr_trace -> shadow rays (ballot compaction) ->
mr_trace_indirect -> Phong shade, for a set of image rows; plus the image-tile sharding and the single
framebuffer gather used on a multi-GPU node.

This replaces the reference's per-pixel recursion (Scene::raytraceImage, Scene.cpp:93-212) by batches;
torch supplies device memory, streams and torch.distributed (backend "nccl" = RCCL) only.
"""
import collections
import contextlib

import numpy as np
import torch

from . import binding, scenes


# ------------------------------------------------------------------------------------------------ sharding
def band_rows(H, band, rank, world):
    """Image rows owned by `rank`: horizontal bands of `band` rows dealt round-robin (interleaved for load
    balance, cf. the reference's `schedule(dynamic, 2)` rows, Scene.cpp:113).  Returns [(y0, y1), ...]."""
    out = []
    nb = (H + band - 1) // band
    for b in range(rank, nb, world):
        out.append((b * band, min(H, (b + 1) * band)))
    return out


def rows_of(bands):
    if not bands:
        return np.zeros(0, np.int64)
    return np.concatenate([np.arange(y0, y1, dtype=np.int64) for y0, y1 in bands])


class FrameGather:
    """The one collective of a frame, with everything that does not change from frame to
    frame set up once: every rank owns a send buffer padded to the largest shard -- the renderer shades straight
    into its leading rows (`local`), so there is no staging copy -- and rank `dst` owns the receive buffer, the
    full frame and the row permutation that de-interleaves the bands.

    `start()` enqueues the gather asynchronously (RCCL runs it on its own stream behind the shading kernel);
    `wait()` makes the caller's stream wait for it and, on `dst`, de-interleaves.  A renderer calls `wait()` just
    before it shades the next frame, so frame k's gather overlaps frame k+1's trace launches."""

    def __init__(self, H, W, band, rank, world, device, dtype=torch.float32, group=None, dst=0, always_collective=False,
                 channels=3, scene=None):
        """always_collective: go through torch.distributed even when world == 1 (exercises the RCCL call on one GPU).
        channels: values per pixel -- 3 for the float framebuffer; 4 * spp gathers the frame's mr_hit records instead
        (the hit-buffer parity mode of SURVEY.md section 8e: 16 bytes per ray, viewed as float32)."""
        # scene: a built miro_amd.Scene on `device`; with it rank `dst` de-interleaves with the library's own kernel
        # (mr_deinterleave_bands, one launch on the current stream) instead of a torch index_select + index_copy_ pair
        self.scene = scene if dtype == torch.float32 else None
        self.channels = C = channels
        self.H, self.W, self.band, self.rank, self.world, self.group, self.dst = H, W, band, rank, world, group, dst
        self.local_only = world == 1 and not always_collective
        self.counts = [sum(y1 - y0 for y0, y1 in band_rows(H, band, r, world)) for r in range(world)]
        self.max_rows = max(self.counts)
        self.send = torch.zeros((max(self.max_rows, 1) * W, C), dtype=dtype, device=device)
        self.local = self.send[:self.counts[rank] * W]            # [n_local_rows * W, C], rows in band order
        self.work = None
        self.pending = False
        self.full = None
        if rank == dst:
            self.recv = self.send.unsqueeze(0) if self.local_only else \
                torch.empty((world, max(self.max_rows, 1) * W, C), dtype=dtype, device=device)
            self.full = torch.empty((H, W, C), dtype=dtype, device=device)
            dest = np.concatenate([rows_of(band_rows(H, band, r, world)) for r in range(world)])
            src = np.concatenate([r * max(self.max_rows, 1) + np.arange(self.counts[r], dtype=np.int64) for r in range(world)])
            self.dest_rows = torch.from_numpy(dest).to(device)
            self.src_rows = torch.from_numpy(src).to(device)

    def _staged(self):
        import torch.distributed as dist
        return not self.local_only and self.send.is_cuda and dist.get_backend(self.group) == "gloo"

    def start(self):
        import torch.distributed as dist
        if self.pending:
            self.wait()
        self.pending = True
        if self.local_only:
            return
        if self._staged():
            # rehearsal of the multi-rank path on a box with fewer GPUs than ranks (MIRO_DIST_BACKEND=gloo): gloo has
            # no CUDA gather, so the shard is staged through the host; the production path is the RCCL branch below
            send_h = self.send.cpu()
            recv_h = [torch.empty_like(send_h) for _ in range(self.world)] if self.rank == self.dst else None
            dist.gather(send_h, recv_h, dst=self.dst, group=self.group)
            if self.rank == self.dst:
                self.recv.copy_(torch.stack(recv_h))
            return
        recv = list(self.recv.unbind(0)) if self.rank == self.dst else None
        self.work = dist.gather(self.send, recv, dst=self.dst, group=self.group, async_op=True)

    def wait(self):
        """Returns the full [H, W, channels] frame on `dst` (valid for work enqueued after this call), None elsewhere."""
        if not self.pending:
            return self.full
        if self.work is not None:
            self.work.wait()
            self.work = None
        self.pending = False
        if self.rank != self.dst:
            return None
        if self.scene is not None and self.recv.is_cuda:
            self.scene.deinterleave_bands(self.recv, self.full, self.W, self.H, self.band, self.world, max(self.max_rows, 1),
                                          self.channels, stream=torch.cuda.current_stream(self.recv.device))
            return self.full
        rows = self.recv.reshape(-1, self.W * self.channels).index_select(0, self.src_rows)
        self.full.view(self.H, self.W * self.channels).index_copy_(0, self.dest_rows, rows)
        return self.full


def gather_framebuffer(local_rgb, H, W, band, rank, world, group=None, dst=0):
    """One-shot form of FrameGather: every rank contributes the rows it rendered ([n_local_rows*W, C] values, rows in
    band order; C = 3 for the framebuffer, 4*spp for hit records viewed as float32); rank `dst` receives them in one
    gather and de-interleaves into [H, W, C]."""
    C = local_rgb.shape[-1]
    g = FrameGather(H, W, band, rank, world, local_rgb.device, local_rgb.dtype, group, dst, channels=C)
    g.local.copy_(local_rgb.reshape(-1, C)[:g.counts[rank] * W])
    g.start()
    return g.wait()


# ------------------------------------------------------------------------------------------------ renderer
class FusedFrame:
    """One rank's share of a direct-light frame rendered by mr_render_direct: a single launch per step, no ray buffers.
    Resident: the float framebuffer shard (12 B per pixel) and, when `keep_hits`, the two hit-record buffers
    (16 + 16 B per sample) that parity tests compare with the batched pipeline's.  With `lights` the launch is
    mr_render_lights: the frame over a light list, and `keep_hits` keeps the primary records only.  On a scene with a texture
    table (Scene.n_textures at step()) that launch is mr_render_lights_surface: the same frame with every hit's looked-up colour
    and bump-mapped normal.  A sample that misses contributes 0 in both: the scene's environment (set_environment) is not
    applied.  With `lights` and `environment` the launch is mr_render_lights_environment on any scene: that frame with the
    environment's value -- bg_color, or the lookup of the full-resolution image -- as the L of every sample that misses, the
    level-0 image of Scene::raytraceImage with its background, still one launch and no ray buffers; d_counts then has five
    words (environment_counts())."""

    def __init__(self, scene, desc, W, H, spp=1, band=None, rank=0, world=1, jitter=None, seed=168, flags=0, rgb=None,
                 tiled=None, keep_hits=False, any_shadow=False, no_shadows=False, lights=None, environment=None):
        """no_shadows: MR_FRAME_NO_SHADOWS, the reference's -DDISABLE_SHADOWS build (primary rays only, BASELINE config 2).
        A scene with a material table (Scene.set_materials) is shaded with its per-object materials (Phong.cpp:99-156).
        lights: a list for Scene.set_lights (point and disc lights), set once here; step() then renders with
        Scene.render_lights instead of the description's one point light (any_shadow: MR_TRACE_ANY for the shadow rays;
        no_shadows is not available there).  None: nothing changes.
        environment (with `lights` only): True -- misses are shaded with the scene's environment as it is set; a dict -- the
        arguments of Scene.set_environment, applied once here; step() then renders with Scene.render_lights_environment.
        None: nothing changes."""
        if isinstance(desc, str):
            desc = scenes.SCENES[desc]
        if lights is not None and no_shadows:
            raise ValueError("FusedFrame: no_shadows is not available with a light list (mr_render_lights always traces shadow rays)")
        if environment is not None and environment is not True and not isinstance(environment, dict):
            raise ValueError("FusedFrame: environment is None, True or a dict of Scene.set_environment's arguments")
        if environment is not None and lights is None:
            raise ValueError("FusedFrame: environment needs a light list (mr_render_direct has no environment)")
        self.lights = None if lights is None else list(lights)
        if self.lights is not None:
            scene.set_lights(self.lights)
        self.environment = environment is not None
        if isinstance(environment, dict):
            scene.set_environment(**environment)
        self.scene, self.desc, self.W, self.H, self.spp = scene, desc, W, H, spp
        self.jitter = (spp > 1) if jitter is None else jitter
        self.seed = seed
        self.flags = flags | (binding.MR_TRACE_ANY if any_shadow else 0) | (binding.MR_FRAME_NO_SHADOWS if no_shadows else 0)
        self.device = torch.device("cuda", scene.device)
        self.bands = (band, rank, world) if world > 1 else None
        self.n_rows = sum(y1 - y0 for y0, y1 in band_rows(H, band, rank, world)) if world > 1 else H
        self.n_pixels = self.n_rows * W
        self.n = self.n_pixels * spp
        self.tiled = (spp < 64) if tiled is None else bool(tiled)
        f32 = dict(dtype=torch.float32, device=self.device)
        self.d_rgb = torch.zeros((max(self.n_pixels, 1), 3), **f32) if rgb is None else rgb
        if self.d_rgb.numel() < 3 * self.n_pixels or self.d_rgb.dtype != torch.float32 or not self.d_rgb.is_contiguous():
            raise ValueError("rgb must be a contiguous float32 buffer of at least %d x 3 values" % self.n_pixels)
        self.d_hits = torch.empty((max(self.n, 1), 4), **f32) if keep_hits else None
        self.d_shadow_hits = torch.empty((max(self.n, 1), 4), **f32) if keep_hits and self.lights is None else None
        # primary rays, shadow rays and, with a light list, undefined lookups (mr_render_direct's counters stay two words: the
        # tests of its counter ring compare the whole tensor); with an environment besides misses and undefined environment lookups
        self.d_counts = torch.zeros(2 if self.lights is None else 5 if self.environment else 3, dtype=torch.int64, device=self.device)
        self.cam = binding.make_camera(desc["eye"], desc["lookat"], desc["up"], desc["fov"])

    def bytes_resident(self):
        own = [self.d_rgb, self.d_counts] + [t for t in (self.d_hits, self.d_shadow_hits) if t is not None]
        return sum(t.numel() * t.element_size() for t in own)

    def step(self, stream=None):
        if self.n == 0:
            return
        if self.lights is not None:
            render = self.scene.render_lights_surface if self.scene.n_textures else self.scene.render_lights
            if self.environment:
                render = self.scene.render_lights_environment
            render(self.cam, self.W, self.H, self.d_rgb, bands=self.bands, spp=self.spp, jitter=self.jitter, seed=self.seed, tiled=self.tiled,
                   flags=self.flags, d_hits=self.d_hits, d_counts=self.d_counts, stream=stream)
            return
        self.scene.render_direct(self.cam, self.W, self.H, self.d_rgb, self.desc["light"], self.desc["wattage"],
                                 bands=self.bands, spp=self.spp, jitter=self.jitter, seed=self.seed, tiled=self.tiled,
                                 flags=self.flags, d_hits=self.d_hits, d_shadow_hits=self.d_shadow_hits,
                                 d_counts=self.d_counts, stream=stream)

    def ray_counts(self, steps=1):
        """(primary, shadow) rays per step, from the device counters accumulated over `steps` steps -- synchronises."""
        c = self.d_counts.cpu().numpy()
        return int(c[0]) // max(steps, 1), int(c[1]) // max(steps, 1)

    def undefined_lookups(self, steps=1):
        """Hits whose texture lookup the reference leaves undefined, per step (mr_render_lights_surface's d_counts[2]; 0 for every
        other launch of this class) -- synchronises."""
        return int(self.d_counts.cpu().numpy()[2]) // max(steps, 1) if self.lights is not None else 0

    def environment_counts(self, steps=1):
        """(misses, undefined environment lookups) per step: mr_render_lights_environment's d_counts[3] and [4]; (0, 0) for
        every other launch of this class -- synchronises."""
        if not self.environment:
            return 0, 0
        c = self.d_counts.cpu().numpy()
        return int(c[3]) // max(steps, 1), int(c[4]) // max(steps, 1)


class Queue(collections.namedtuple("Queue", "rays weights pixels ids octs n low", defaults=(None,))):
    """One level's rays in render_specular: weights and pixels (None: the eye rays, weight 1 and pixel = ray index // spp),
    the path tracer's ray ids and the octant bytes (None where the plan has none), the number of rays, and (fused="lights_path"
    only) one byte per ray that is non-zero for a ray made by Ray::random."""
    __slots__ = ()

    def first(self, n):
        """the leading n rays of freshly generated children"""
        rays, weights, pixels, ids, octs, _, low = self
        return Queue(rays[:n], weights[:n], pixels[:n], ids if ids is None else ids[:n], octs if octs is None else octs[:n], n,
                     low if low is None else low[:n])


NO_QUEUE = Queue(None, None, None, None, None, 0)


# One value of render_specular's `fused` as independent choices.
# driver: who runs level 0 and the loop -- "queue" (generate()'s rays, one step per level), "frame" (_frame_level0, then
# _level_lights) or "device" (_device_levels: one library call);
# level: the level form -- "batched", "point" (mr_trace_level), "auto" (point where the queue hits, else batched) or "lights"
# (mr_trace_level_lights / _path); besides, "unlisted" for a truthy `fused` outside the table (route_of): checked like "point",
# run like "batched";
# path: the _path kernel form of "lights" (the batched path takes it from path_tracing); lens: level 0 goes through the thin
# lens; photons: the maps go into the one device call.
Route = collections.namedtuple("Route", "driver level path lens photons", defaults=(False, False, False))

# every accepted value of `fused`; this table is the only place that knows the strings
ROUTES = {
    False: Route("queue", "batched"),
    True: Route("queue", "point"),
    "auto": Route("queue", "auto"),
    "lights": Route("queue", "lights"),
    "lights_path": Route("queue", "lights", path=True),
    "frame_lights": Route("frame", "lights"),
    "frame_lights_path": Route("frame", "lights", path=True),
    "device_lights": Route("device", "lights"),
    "device_lights_path": Route("device", "lights", path=True),
    "device_photons": Route("device", "lights", photons=True),
    "device_photons_path": Route("device", "lights", path=True, photons=True),
    "frame_lens": Route("frame", "lights", lens=True),
    "frame_lens_path": Route("frame", "lights", path=True, lens=True),
    "device_lens": Route("device", "lights", lens=True),
    "device_lens_path": Route("device", "lights", path=True, lens=True),
    "device_lens_photons": Route("device", "lights", lens=True, photons=True),
    "device_lens_photons_path": Route("device", "lights", path=True, lens=True, photons=True),
}
ROUTES_BY_FIELDS = {route: name for name, route in ROUTES.items()}      # a route's name, as the messages print it
QUEUE_FORM = dict(driver="queue", lens=False, photons=False)            # the fields that make a route its per-level sibling


def route_of(fused):
    """ROUTES[fused].  A value outside the table keeps what it always did: a falsy one is the batched path; any other passes
    mr_trace_level's checks as a truthy `fused` and then runs the batched steps (level "unlisted")."""
    if isinstance(fused, (bool, str)) and fused in ROUTES:
        return ROUTES[fused]
    return Route("queue", "unlisted" if fused else "batched")


class LevelPlan(collections.namedtuple("LevelPlan", (
        "stream", "flags", "route", "path_tracing", "path_kinds", "fan", "path_seed", "group_octants", "lights", "environment",
        "env_lowres", "surface", "square", "square_lights", "surface_children", "photon_maps", "nphotons", "max_dist", "lens"))):
    """What FrameRenderer.render_specular decides once per call, from its arguments and the scene's state (_resolve):
    stream: the torch Stream of every launch, None for the current one; flags: the renderer's trace flags;
    route: the Route of `fused`; its level is already "batched" where a scene with a texture table turned "point" or "auto" away;
    path_tracing, path_kinds (never None), fan (children per ray, at most), path_seed, group_octants: as given;
    lights: the scene's light list shades, not the description's point light; environment: misses are shaded, after the
    first level with env_lowres (MR_ENV_LOWRES or 0);
    surface: the scene has a procedural texture, so shading reads the surface pass's colour and normal;
    square: None, "plain" (mr_shade_square_lights) or "surface" (any texture table), for square_lights;
    surface_children: the path tracer's children come from mr_gen_path_rays_surface;
    photon_maps: None or (global, caustic), gathered with nphotons / max_dist; lens: the renderer's lens on a lens route, else None."""
    __slots__ = ()

    def surface_pass(self, last):
        """does a level run mr_hit_surface: for its shading, for its square lights, or for its children (not the last level's)"""
        return self.surface or self.square == "surface" or (self.surface_children and not last)

    def level_flags(self, level, grouped=False):
        """The flag words of a level: (trace batches, shading calls, mr_trace_level / mr_trace_grouped).  Bounce queues are
        compacted in wave order, not in image order: from the first bounce on they carry the MR_TRACE_INCOHERENT hint (voting
        control flow; the same hit records), except where the level works through an octant order (`grouped`)."""
        hint = binding.MR_TRACE_INCOHERENT if level > 0 else 0
        trace = self.flags | hint
        return (trace, trace & (binding.MR_MATH_PRODUCT | binding.MR_TRACE_INCOHERENT),
                (self.flags & binding.MR_MATH_PRODUCT) | (0 if grouped else hint))


class FrameRenderer:
    """All device buffers of one rank's share of a frame, resident for the lifetime of the object."""

    def __init__(self, scene, desc, W, H, spp=1, bands=None, jitter=None, seed=168, flags=0, device=None, rgb=None,
                 tiled=None, lens=None, square_lights=None, square_samples=1, resident_rays=True):
        """lens: dict(aperture, focus_plane) -- generate() then makes the eye rays of the thin-lens camera
        (mr_gen_eye_rays_lens, Camera::eyeRay under -DDOF) in image order; not with tiled=True.  render_specular's fused="frame_lens*" |
        "device_lens*" routes make the same rays inside the fused frame and need it.
        square_lights: a list of SquareLights (binding.SquareLightDesc objects or dicts) that every level of render_specular's
        batched path shades IN ADDITION to its point light / light list, with square_samples shadow rays per hit and light
        (mr_shade_square_lights; level l draws its pairs with seed + l; on a scene with a texture table, procedural or not,
        mr_hit_surface and mr_shade_square_lights_surface with the same seeds).  Without either option nothing changes.
        resident_rays=False: the ray, hit and shadow buffers (100 bytes per sample) are not allocated; what is left serves
        render_specular(fused="frame_lights" | "frame_lights_path") without photon maps and fused="device_*", whose level 0 keeps
        its rays in registers.  Every method that needs those buffers then raises ValueError."""
        if isinstance(desc, str):
            desc = scenes.SCENES[desc]
        self.scene, self.desc, self.W, self.H, self.spp = scene, desc, W, H, spp
        self.lens, self.square_lights, self.square_samples = lens, square_lights, square_samples
        if lens is not None and tiled:
            raise ValueError("FrameRenderer: lens eye rays come in image order only (tiled must be falsy)")
        self.bands = bands if bands is not None else [(0, H)]
        self.jitter = (spp > 1) if jitter is None else jitter
        self.seed, self.flags = seed, flags
        self.device = torch.device("cuda", scene.device) if device is None else device
        self.n_rows = sum(y1 - y0 for y0, y1 in self.bands)
        self.n_pixels = self.n_rows * W
        self.n = self.n_pixels * spp
        n = max(self.n, 1)
        f32 = dict(dtype=torch.float32, device=self.device)
        self.resident_rays = bool(resident_rays)
        self.d_rays = self.d_hits = self.d_shadow_rays = self.d_shadow_hits = self.d_src = None
        if self.resident_rays:
            self.d_rays = torch.empty((n, 8), **f32)
            self.d_hits = torch.empty((n, 4), **f32)
            self.d_shadow_rays = torch.empty((n, 8), **f32)
            self.d_shadow_hits = torch.empty((n, 4), **f32)
            self.d_src = torch.empty(n, dtype=torch.int32, device=self.device)
        self.d_count = torch.zeros(1, dtype=torch.int64, device=self.device)
        self.d_gather = None                            # final_gather's scratch, allocated on first use
        self.d_recursion = self.d_level_counts = None   # mr_render_recursion's workspace and counters, allocated on first use
        self.d_pass_counts = self.d_bytes = None        # mr_render_recursion_passes' counters, finish()'s bytes: likewise
        # rgb: an external [n_pixels, 3] buffer to shade into (FrameGather.local on a multi-GPU node)
        self.d_rgb = torch.zeros((max(self.n_pixels, 1), 3), **f32) if rgb is None else rgb
        self.cam = binding.make_camera(desc["eye"], desc["lookat"], desc["up"], desc["fov"])
        # Below 64 samples per pixel the rays can be generated in the tiled order of mr_gen_eye_rays_tiled (a wave covers a
        # square of pixels instead of a strip); tracing, shadow rays and shading are order-agnostic and work on pixel
        # SLOTS, and the shaded slots are scattered to image order (d_rgb) with the window's pixel map.
        # tiled=None: image order (ray k belongs to pixel k // spp in row-major order, what callers indexing d_rays /
        # d_hits expect); tiled=True is the fast choice for whole frames
        self.tiled = bool(tiled) and spp < 64 and spp & (spp - 1) == 0
        if self.tiled and self.n_pixels:
            maps, off = [], 0
            for y0, y1 in self.bands:
                maps.append(binding.tile_pixel_map(W, y1 - y0, spp).astype(np.int64) + off)
                off += (y1 - y0) * W
            self.d_slot_pixel = torch.from_numpy(np.concatenate(maps)).to(self.device)
            self.d_slots = torch.zeros((self.n_pixels, 3), **f32)
        else:
            self.tiled = False
            self.d_slots = self.d_rgb

    def bytes_resident(self):
        own = [self.d_rays, self.d_hits, self.d_shadow_rays, self.d_shadow_hits, self.d_src, self.d_count, self.d_rgb]
        if self.tiled:
            own += [self.d_slots, self.d_slot_pixel]
        own += [self.d_recursion, self.d_level_counts, self.d_pass_counts, self.d_bytes]
        return sum(t.numel() * t.element_size() for t in own if t is not None)

    def _need_rays(self, what):
        if not self.resident_rays:
            raise ValueError("FrameRenderer: %s needs the resident ray, hit and shadow buffers (resident_rays=True)" % what)

    def generate(self, stream=None):
        """Camera::eyeRay for every owned row; the rays then stay resident in HBM."""
        self._need_rays("generate()")
        off = 0
        for y0, y1 in self.bands:
            k = (y1 - y0) * self.W * self.spp
            if self.lens is not None:
                self.scene.gen_eye_rays_lens(self.cam, self.W, self.H, self.d_rays[off:off + k], self.lens["aperture"],
                                             self.lens["focus_plane"], y0=y0, y1=y1, spp=self.spp, jitter=self.jitter,
                                             seed=self.seed, stream=stream)
            else:
                self.scene.gen_eye_rays(self.cam, self.W, self.H, self.d_rays[off:off + k], y0=y0, y1=y1, spp=self.spp,
                                        jitter=self.jitter, seed=self.seed, stream=stream, tiled=self.tiled)
            off += k

    def trace_primary(self, stream=None):
        self._need_rays("trace_primary()")
        self.scene.trace_device(self.d_rays, self.n, self.d_hits, self.flags, stream=stream)

    def make_shadow_rays(self, stream=None):
        self._need_rays("make_shadow_rays()")
        self.scene.gen_shadow_rays(self.d_rays, self.d_hits, self.n, self.desc["light"], self.d_shadow_rays, self.d_src,
                                   self.d_count, stream=stream)

    def trace_shadow(self, stream=None, any_hit=False):
        self._need_rays("trace_shadow()")
        fl = self.flags | (binding.MR_TRACE_ANY if any_hit else 0)
        self.scene.trace_indirect(self.d_shadow_rays, self.d_count, self.n, self.d_shadow_hits, fl, stream=stream)

    def _untile(self, stream=None):
        """slot order -> image order (a no-op for frames generated in image order): the library's own scatter, band by
        band, on the caller's stream (whatever kind of handle it is)"""
        if not self.tiled:
            return
        off = 0
        for y0, y1 in self.bands:
            k = (y1 - y0) * self.W
            self.scene.untile_pixels(self.d_slots[off:off + k], self.d_rgb[off:off + k], self.W, y1 - y0, self.spp, channels=3,
                                     stream=stream)
            off += k

    def shade(self, stream=None):
        self._need_rays("shade()")
        self.scene.shade_direct(self.d_rays, self.d_hits, self.n, self.d_shadow_hits, self.d_src, self.d_count,
                                self.desc["light"], self.desc["wattage"], self.d_slots, spp=self.spp, stream=stream)
        self._untile(stream)

    def final_gather(self, global_map, caustic_map=None, nphotons=500, max_dist=1e10, stream=None):
        """BASELINE config 5: the photon-map term of Scene::traceScene (Scene.cpp:285-299) for the primary hits of this
        frame, added to d_rgb after `step()`.  The scratch (48 B per ray) is allocated on first use."""
        self._need_rays("final_gather()")
        if self.n == 0:
            return
        if self.d_gather is None:
            self.d_gather = torch.empty(12 * self.n, dtype=torch.float32, device=self.device)
        self.scene.final_gather(global_map, caustic_map, self.d_rays, self.d_hits, self.n, self.d_gather, self.d_slots,
                                max_dist=max_dist, nphotons=nphotons, spp=self.spp, stream=stream)
        self._untile(stream)

    def step(self, stream=None, any_hit=False):
        """One pass of the hot path over this rank's resident rays: primary batch, shadow batch, shade."""
        self._need_rays("step()")
        if self.n == 0:
            return
        self.trace_primary(stream)
        self.make_shadow_rays(stream)
        self.trace_shadow(stream, any_hit)
        self.shade(stream)

    def capture(self, any_hit=False):
        """One frame step recorded into a HIP graph (torch.cuda.CUDAGraph): small frames are launch-bound -- five
        kernels and a memset of tens of microseconds each -- and replay as one submission.  The step must have run
        once before (the library's grow-only scratch buffers are sized outside the capture).  Returns the graph;
        `graph.replay()` re-renders into d_rgb."""
        self._need_rays("capture()")
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        side = torch.cuda.Stream(device=self.device)
        side.wait_stream(torch.cuda.current_stream(self.device))
        with torch.cuda.stream(side):
            self.step(side, any_hit)            # warm-up on the capture stream
        torch.cuda.current_stream(self.device).wait_stream(side)
        torch.cuda.synchronize()
        with torch.cuda.graph(g, stream=side):
            self.step(torch.cuda.current_stream(self.device), any_hit)
        return g

    def render_specular(self, depth=10, stream=None, path_tracing=False, path_seed=168, path_kinds=None, fused=False,
                        group_octants=False, lights=None, environment=None, photon_maps=None, nphotons=500, max_dist=1e10,
                        surface_children=None, queue_capacity=None, samples=None):
        """Scene::traceScene with reflective / refractive materials (Scene.cpp:270-346) as wavefront bounces: every
        level traces its queue, shades it (weight x Phong::shade added to the ray's pixel), and emits the reflect /
        Fresnel / refract children of the next level by ballot compaction.  depth = TRACE_DEPTH (Miro.h:13): rays are
        traced while depth >= 0, i.e. up to depth+1 levels.  Returns the number of rays traced per level.
        path_tracing: the PATH_TRACING build of the generators (mr_gen_path_rays: lobe-sampled children, Ray.h:149-158,
        235-239; path_kinds |= MR_PATH_DIFFUSE adds Ray::random's bounce, an extension) with stable ray ids handed down
        the levels so that every child's random numbers are those of the oracle's recursion.
        fused: every level is ONE launch of mr_trace_level (trace, shadow ray, trace, shade, children) instead of the seven
        of the batched calls -- the same rays and children; no hit or shadow-ray buffer exists.  fused="auto": the first
        level in one launch, a later level only if at least 90 % of the previous level's rays hit something (the one-launch
        form runs its second traversal and its generators at the hit rate of the queue, profiles/r02_level_probe.log).
        group_octants: the generators also write one octant byte per child, and every level after the first works on its
        queue through mr_order_by_octant's index (rays grouped by direction octant inside chunks of 16 384; the same hits and
        children).  Off by default: the bounce rays' own traversal gains 9-13 %, the frame does not (the shadow rays of grouped
        lanes are no more coherent, the pixel runs of accumulate_runs break up, profiles/r03_octant_order.log).
        lights: a light list (binding.LightDesc objects or the dicts of scenes.py, point and disc lights) instead of the
        description's single point light: it becomes the scene's list (Scene.set_lights) and every level is trace ->
        mr_shade_lights -> the generators, three launches without shadow-ray buffers.  The first level's hits stay in d_hits
        (final_gather works on them).  `fused` must be falsy: mr_trace_level keeps its single point light.
        environment: what a ray that leaves the scene is worth (Scene::getEnvironmentMap, Scene.cpp:338-342,657-688): a dict
        with bg_color / pixels / rotation (the arguments of Scene.set_environment; it becomes the scene's), or True for the
        environment the scene already has.  Every level, the last one included (traceScene at depth 0 still traces and
        still returns the environment), then calls mr_shade_environment on its queue after tracing it.  `fused` must be
        falsy: mr_trace_level keeps no hit records.  The low-res image (the reference's ray.isDiffuse) is used for every level
        after the first when path_kinds == MR_PATH_DIFFUSE and never for specular children; with an IMAGE, MR_PATH_DIFFUSE
        mixed with other kinds is refused (the child queue does not record which child came from Ray::random).  None: a miss
        is worth 0 and no launch is added.
        A scene with a texture table (Scene.set_textures) takes the batched path for every level, whatever `fused` says
        (fused="auto" included): mr_trace_level shades without the texture lookup and refuses such a scene; the batched
        path's mr_shade_accumulate / mr_shade_lights look the diffuse colour up (Phong.cpp:51-56).
        A scene whose table holds a procedural texture (a StoneTexture or a StemTexture, or one of the UVW kinds PetalTexture,
        LeafTexture, FlowerCenterTexture, which are looked up at the hit point itself) adds one launch per level: trace ->
        mr_hit_surface (diffuse colour and bump-mapped normal of every hit into two [n, 3] buffers sized to the level's queue)
        -> mr_shade_lights_surface (light list) or the shadow batch and mr_shade_accumulate_surface (single light) -> the
        generators.
        surface_children: under path_tracing, a level's children come from mr_gen_path_rays_surface, which reads the level's
        colour and normal buffers: every child bounces about the normal Scene::trace hands on (the bumped one on stone) and the
        diffuse child carries weight x diffuseColor, the looked-up colour (Phong.cpp:51-56), not the material's m_diffuse.  None:
        on a scene with a procedural texture, and only there.  True: on any scene; a level whose surface pass does not run
        already gets it (mr_hit_surface works with or without a table), and `fused` must be falsy on a scene without a table.
        False: mr_gen_path_rays everywhere, which refuses MR_PATH_DIFFUSE on a scene with a procedural texture (ValueError here,
        before any launch).  Without path_tracing it has no effect: the non-path generators emit no diffuse child.
        Square lights (FrameRenderer(square_lights=...)) on a scene with any texture table, checker and image textures included,
        are shaded by mr_shade_square_lights_surface(seed + level) from the level's colour and normal buffers; where the table
        holds no procedural texture, mr_hit_surface is launched for them alone and the other calls of the level stay the
        textured ones.  On a scene without a table it is mr_shade_square_lights, as before, and no surface pass.
        photon_maps: (global, caustic) binding.PhotonMap objects, balanced and resident; either may be None.  The photon-map
        term of Scene::traceScene (Scene.cpp:286-299) at EVERY level: after a level is traced and shaded and before its
        children are generated, mr_gather_level runs on the level's queue with its weights and pixels -- irradiance_estimate of
        both maps at every diffuse hit, weight x (irradiance + caustic) / spp added to the ray's pixel -- so a diffuse wall seen
        in a mirror or through glass carries its indirect light and its caustics.  nphotons / max_dist: PHOTON_SAMPLES and
        PHOTON_MAX_DIST (Miro.h:16-17).  On a scene with a procedural texture the queries take the normal buffer that
        mr_hit_surface just filled (the bumped normal, Scene.cpp:290), otherwise the object's normal.  The scratch (12 floats per
        ray) is allocated with the level's other buffers.  `fused` must be falsy: mr_trace_level keeps no hit records.  None: no
        launch is added.
        The routes.  Besides False, True and "auto", `fused` takes 14 strings.  Each is one combination of five independent
        choices, the fields of frame.Route; frame.ROUTES is the table at the end.  All 14 are opt-in: fused="auto" never chooses
        one (a level whose rays rarely hit runs its light loop at that lane utilisation; DESIGN section 5c has the times).
        driver -- who runs level 0 and the loop:
          "queue": generate()'s eye rays are level 0's queue, d_slots is zeroed, one step per level (the level form below), each
            with its counters and queue allocated before it and its child count read back after it, then the untile pass.  It
            needs the resident ray buffers, and serves a lens (generate() makes lens rays), tiled=True and any number of band ranges.
          "frame": level 0 is ONE mr_render_level_lights straight into d_rgb -- the fused frame that also writes the rays of level 1:
            no generate(), no zeroing of the pixels, no eye-ray buffer, no atomics at level 0 (its pixels are deterministic) and no
            untile pass (the children's pixels index d_rgb, in image order, also with tiled=True) -- and the levels >= 1 are
            mr_trace_level_lights / _path on the children, adding into d_rgb.  One window per call: ValueError for more than one
            band range (the "queue" driver takes them).  photon_maps= are taken (image order only: ValueError with tiled=True, which
            needs tiled=False or the "queue" driver): generate() then runs as well, for mr_gather_level's level 0; without maps a
            FrameRenderer(resident_rays=False) serves.  The same rays, children and counts per level as the "queue" driver; level 0's
            pixel means are pairwise sums where that one adds atomically.
          "device": that frame as ONE library call, mr_render_recursion, followed by ONE read of its counters: level 0 as there,
            every further level one kernel that reads the length of its queue from the count the level before left on the device.
            No read-back, allocation or torch op between the levels (Scene.render_recursion alone can be captured into a graph); a
            FrameRenderer(resident_rays=False) serves.  The checks of "frame", and ValueError besides with photon_maps unless
            photons is set (the "frame" driver takes them: mr_gather_level takes its n from the host).
            queue_capacity: rays per queue, None: fan x samples (3 specular, 4 path traced), which always holds level 1; a level that
            emits more children than that is truncated, and the call raises RuntimeError naming the level, its children and the
            capacity (fan^depth x samples can never be exceeded).  The workspace (two queues) and the counters are allocated on
            first use and kept (bytes_resident counts them).  The same rays, children and counts per level as the "frame" driver,
            cut at the first level with 0 rays; the pixel sums of levels >= 1 differ by the order of the float atomics.
        level -- the form of a level ("frame" and "device" exist for "lights" only):
          "batched" (False), "point" (True: mr_trace_level, one point light) and "auto": above.  A truthy value outside the table
            is "unlisted": it passes the checks of "point" and then runs the batched steps; a falsy one is "batched".
          "lights": every level is ONE launch of mr_trace_level_lights on ANY scene -- trace, the environment of a miss, the surface
            step (texture table or none, bumped normal), the loop over the light list, weight x L to the pixel, the specular children
            -- where the batched path runs trace -> mr_shade_environment -> mr_hit_surface -> mr_shade_lights[_surface] ->
            mr_gen_secondary_rays.  It needs lights=[...], takes environment= in every form and photon_maps= (the launch then also
            writes the level's hit records, and bumped normals on a procedural scene, and mr_gather_level follows it), and raises
            ValueError with path_tracing, square lights, group_octants or surface_children=True.  The same rays, children and counts
            as the batched path; the pixel sums differ by the order of the float atomics.
        path -- the same for a PATH_TRACING build: every level is ONE launch of mr_trace_level_lights_path, whose children are those
          of mr_gen_path_rays_surface (about the bumped normal, the diffuse child with the looked-up colour) -- the batched path with
          surface_children=True.  It needs lights=[...] and path_tracing=True, takes environment=, photon_maps=, path_seed and
          path_kinds, and raises ValueError with square lights, group_octants or surface_children=False.  Its queues carry the ray
          ids and, with an environment, one byte per ray that marks the children of Ray::random: a miss of such a ray reads the
          low-res image, so an environment IMAGE with MR_PATH_DIFFUSE mixed with other kinds is accepted on these routes.
        lens -- the "frame" or "device" driver of a FrameRenderer(lens=dict(aperture=..., focus_plane=...)): level 0 is ONE
          mr_render_level_lights_lens (inside the one call: mr_render_recursion_lens, mr_render_recursion_photons_lens), the fused
          frame whose eye rays go through the thin lens (Camera::eyeRay under -DDOF, the rays generate() makes for the same lens,
          made in registers); the further levels, the checks, queue_capacity, the workspace and the truncation rule are the pinhole
          twin's.  With photon_maps on the "frame" driver generate() runs for mr_gather_level's level 0: it already makes lens rays.
          ValueError besides without a lens (naming the pinhole route) and with tiled=True; the pinhole routes go on refusing a lens
          (the batched path or the "queue" driver takes it).  The same rays, children and counts per level as the batched lens
          frame (fused="lights" / "lights_path").
        photons -- the "device" driver WITH photon_maps=(global, caustic), as ONE mr_render_recursion_photons and one read of its
          counters: after every level the photon-map term of that level's queue (mr_gather_level's queries, estimates and adds) by
          kernels that read the queue's length from the device too.  nphotons, max_dist and queue_capacity as above; the workspace
          also holds a level's hit records, normals and the scratch of the estimates.  ValueError without photon_maps (naming the
          route without photons), with tiled=True ("lights" / "lights_path", or tiled=False), and with what the "device" driver
          refuses.  The same rays, children, queries and counts per level as the "frame" driver with the same maps; pixel sums
          differ by the order of the float atomics.
          fused                        driver  level    path lens photons  refuses (ValueError), besides a missing light list
          False                        queue   batched  -    -    -        (what each option above says)
          True                         queue   point    -    -    -        photon_maps, surface_children, environment, lights, square lights
          "auto"                       queue   auto     -    -    -        as True
          "lights"                     queue   lights   -    -    -        path_tracing, square lights, group_octants, surface_children=True
          "lights_path"                queue   lights   yes  -    -        no path_tracing, square lights, group_octants, surface_children=False
          "frame_lights"               frame   lights   -    -    -        as "lights"; a lens, two band ranges, maps with tiled=True
          "frame_lights_path"          frame   lights   yes  -    -        as "lights_path"; the same three
          "device_lights"              device  lights   -    -    -        as "frame_lights"; photon_maps
          "device_lights_path"         device  lights   yes  -    -        as "frame_lights_path"; photon_maps
          "device_photons"             device  lights   -    -    yes      as "frame_lights"; no photon_maps, tiled=True
          "device_photons_path"        device  lights   yes  -    yes      as "frame_lights_path"; no photon_maps, tiled=True
          "frame_lens"                 frame   lights   -    yes  -        as "frame_lights" but for the lens; no lens, tiled=True
          "frame_lens_path"            frame   lights   yes  yes  -        as "frame_lights_path" but for the lens; no lens, tiled=True
          "device_lens"                device  lights   -    yes  -        as "device_lights" but for the lens; no lens, tiled=True
          "device_lens_path"           device  lights   yes  yes  -        as "device_lights_path" but for the lens; no lens, tiled=True
          "device_lens_photons"        device  lights   -    yes  yes      as "device_photons" but for the lens; no lens
          "device_lens_photons_path"   device  lights   yes  yes  yes      as "device_photons_path" but for the lens; no lens
        On a scene with a texture table True and "auto" are False (above); the 14 strings are unchanged by it.
        samples=S (fused="device_*" only; any other route raises ValueError): the frame has S samples per pixel, of any number,
        rendered by ONE mr_render_recursion_passes (on a photons route mr_render_recursion_photons_passes) in passes of the
        renderer's spp, the remainder as powers of two (binding.passes_plan) -- sample s of a pixel has the key, the path hash and
        the child ids of a single launch at spp = S, whatever the pass size.  The workspace and queue_capacity are those of ONE
        pass.  Returns per_level summed over the passes; RuntimeError names the first truncated pass.  The jitter is the
        renderer's: FrameRenderer(spp=1, jitter=True) for one-sample passes.  Without `samples` nothing changes."""
        if samples is not None and route_of(fused).driver != "device":
            raise ValueError("render_specular: samples=%r needs a fused=\"device_*\" route (mr_render_recursion_passes); the other "
                             "routes render the renderer's spp samples per pixel" % (samples,))
        plan = self._resolve(stream, path_tracing, path_seed, path_kinds, fused, group_octants, lights, environment, photon_maps,
                             nphotons, max_dist, surface_children)
        # this driver mixes library launches (on `stream`) with torch ops and .item() read-backs: they only order against
        # each other on torch's current stream, so a torch Stream is made current here
        with contextlib.nullcontext() if stream is None else torch.cuda.stream(stream):
            if plan.route.driver == "frame":
                return self._frame_levels(plan, depth)
            if plan.route.driver == "device":
                return self._device_levels(plan, depth, queue_capacity, samples)
            self._need_rays("render_specular(fused=%r)" % (fused,))
            self.d_slots.zero_()
            queue = Queue(self.d_rays, None, None, None, None, self.n)      # the eye rays, in image order
            per_level = []
            for level in range(depth + 1):
                if queue.n == 0:
                    break
                form = plan.route.level
                one_launch = form == "point" or (form == "auto" and (level == 0 or per_level[-1][1] >= 0.9 * per_level[-1][0]))
                step = self._level_lights if form == "lights" else self._level_fused if one_launch else self._level_batched
                counts, queue = step(plan, queue, level, level == depth)
                per_level.append(counts)
            self._untile(stream)
        return per_level

    def _resolve(self, stream, path_tracing, path_seed, path_kinds, fused, group_octants, lights, environment, photon_maps,
                 nphotons, max_dist, surface_children):
        """render_specular's arguments and the scene's state as a LevelPlan: every check, and the two scene setters
        (set_environment, set_lights) between them"""
        sc, route, maps = self.scene, route_of(fused), photon_maps is not None
        name = lambda **changed: ROUTES_BY_FIELDS[route._replace(**changed)]   # noqa: E731  the route's name, or a sibling's
        if route.lens:
            if self.lens is None:
                raise ValueError("render_specular: fused=\"%s\" needs FrameRenderer(lens=dict(aperture=..., focus_plane=...)); "
                                 "the pinhole frame is fused=\"%s\"" % (name(), name(lens=False)))
            if self.tiled:
                raise ValueError("render_specular: fused=\"%s\" needs tiled=False (lens eye rays come in image order only)" % name())
        if route.driver != "queue":
            # level 0 is mr_render_level_lights[_lens]: one window of eye rays, whose children carry image-order pixels
            if route.photons and not maps:
                raise ValueError("render_specular: fused=\"%s\" needs photon_maps=(global, caustic); without maps the frame is "
                                 "fused=\"%s\"" % (name(), name(photons=False)))
            if route.photons and self.tiled:
                raise ValueError("render_specular: photon_maps with tiled=True need fused=\"%s\" (or tiled=False), not "
                                 "fused=\"%s\" (mr_render_recursion_photons finds level 0's pixels from the sample index, in "
                                 "image order)" % (name(**QUEUE_FORM), name()))
            if route.driver == "device" and maps and not route.photons:
                raise ValueError("render_specular: photon_maps need fused=\"%s\", not fused=\"%s\" (mr_gather_level takes the "
                                 "length of its queue from the host)" % (name(driver="frame"), name()))
            if self.lens is not None and not route.lens:
                raise ValueError("render_specular: lens eye rays need the batched path (fused=False), not fused=\"%s\" "
                                 "(mr_render_level_lights makes pinhole eye rays)" % name())
            if len(self.bands) > 1:
                raise ValueError("render_specular: more than one band range needs fused=\"%s\", not fused=\"%s\" "
                                 "(mr_render_level_lights renders one window per call)" % (name(**QUEUE_FORM), name()))
            if maps and self.tiled:
                raise ValueError("render_specular: photon_maps with tiled=True need fused=\"%s\" (or tiled=False), not fused=\"%s\" "
                                 "(mr_gather_level finds level 0's pixels from the ray index, in image order)" % (name(**QUEUE_FORM), name()))
            if maps and route.driver == "frame":
                self._need_rays("render_specular(fused=\"%s\", photon_maps=...)" % name())
        if route.level == "lights":
            call = "mr_trace_level_lights_path" if route.path else "mr_trace_level_lights"
            if lights is None:
                raise ValueError("render_specular: fused=\"%s\" needs lights=[...] (%s shades by the scene's light list)"
                                 % (name(**QUEUE_FORM), call))
            if route.path and not path_tracing:
                raise ValueError("render_specular: fused=\"%s\" needs path_tracing=True (the specular children are fused=\"%s\")"
                                 % (name(**QUEUE_FORM), name(path=False, **QUEUE_FORM)))
            refused = [("path_tracing", path_tracing and not route.path), ("square lights", self.square_lights),
                       ("group_octants", group_octants), ("surface_children=%s" % (not route.path), surface_children is (not route.path))]
            for what, given in refused:
                if given:
                    raise ValueError("render_specular: %s needs the batched path, not fused=\"%s\" (%s emits the %s and shades point "
                                     "and disc lights only)" % (what, name(**QUEUE_FORM), call,
                                                                "children of mr_gen_path_rays_surface" if route.path else "specular children"))
        if sc.n_textures and route.level != "lights":
            route = ROUTES[False]                       # mr_trace_level refuses a texture table
        point = route.level in ("point", "auto", "unlisted")    # the checks below speak of mr_trace_level
        if photon_maps is not None:
            if point:
                raise ValueError("render_specular: photon maps need fused=False (mr_trace_level keeps no hit records)")
            global_map, caustic_map = photon_maps
            photon_maps = (global_map, caustic_map)
        surface = bool(sc.procedural)
        # a reflective STONE material (Scene.bumped_specular; `is True`: a stand-in scene answers every name with a method): the
        # mirror child bounces about the bumped normal, so under path tracing the children are mr_gen_path_rays_surface's
        bumped = sc.bumped_specular is True
        if bumped and path_tracing and surface_children is not None and not surface_children:
            raise ValueError("render_specular: surface_children=False on a scene with a reflective STONE material "
                             "(Scene.bumped_specular: the mirror child bounces about the bump-mapped normal, which mr_gen_path_rays "
                             "does not have; it refuses the scene)")
        if surface_children is None:
            surface_children = surface
        elif not surface_children and surface and path_tracing and path_kinds is not None and path_kinds & binding.MR_PATH_DIFFUSE:
            raise ValueError("render_specular: surface_children=False with MR_PATH_DIFFUSE on a scene with a procedural texture "
                             "(mr_gen_path_rays bounces about the un-bumped normal and refuses the scene)")
        surface_children = bool(surface_children) and path_tracing
        if surface_children and point:
            raise ValueError("render_specular: surface_children needs fused=False (mr_trace_level keeps no hit records)")
        env_lowres = 0
        if environment is not None and environment is not False:
            if point:
                raise ValueError("render_specular: an environment needs fused=False (mr_trace_level keeps no hit records)")
            if environment is not True:
                sc.set_environment(**environment)
            has_image = sc.get_environment(0)[0] is not None
            kinds = binding.MR_PATH_MIRROR | binding.MR_PATH_REFRACT if path_kinds is None else path_kinds
            diffuse_children = path_tracing and bool(kinds & binding.MR_PATH_DIFFUSE)
            if has_image and diffuse_children and kinds != binding.MR_PATH_DIFFUSE and not (route.level == "lights" and route.path):
                raise ValueError("render_specular: an environment image with MR_PATH_DIFFUSE mixed with other kinds "
                                 "(the queue does not record which child came from Ray::random)")
            if diffuse_children and kinds == binding.MR_PATH_DIFFUSE:
                env_lowres = binding.MR_ENV_LOWRES
            environment = True
        else:
            environment = False
        if lights is not None:
            if point:
                raise ValueError("render_specular: a light list needs fused=False (mr_trace_level shades by one point light)")
            sc.set_lights(lights)
        if self.square_lights and point:
            raise ValueError("render_specular: square lights need fused=False (mr_trace_level keeps no hit records)")
        if stream is not None and not isinstance(stream, torch.cuda.Stream):
            raise TypeError("render_specular: pass a torch.cuda.Stream (or None for the current stream), not a raw handle")
        # square lights on a texture table of any kind read the surface pass's buffers (mr_shade_square_lights refuses the table)
        square = None if not self.square_lights else "surface" if sc.n_textures else "plain"
        return LevelPlan(stream=stream, flags=self.flags, route=route, path_tracing=path_tracing,
                         path_kinds=binding.MR_PATH_MIRROR | binding.MR_PATH_REFRACT if path_kinds is None else path_kinds,
                         fan=4 if path_tracing else 3, path_seed=path_seed, group_octants=group_octants, lights=lights is not None,
                         environment=environment, env_lowres=env_lowres, surface=surface, square=square,
                         square_lights=self.square_lights, surface_children=surface_children, photon_maps=photon_maps,
                         nphotons=nphotons, max_dist=max_dist, lens=self.lens if route.lens else None)

    def _children(self, plan, n):
        """The buffers for the children of a level of n rays, at most plan.fan each: ids under path tracing only, octant bytes
        with group_octants only."""
        m, dev = plan.fan * n, self.device
        return Queue(torch.empty((m, 8), dtype=torch.float32, device=dev), torch.empty((m, 3), dtype=torch.float32, device=dev),
                     torch.empty(m, dtype=torch.int32, device=dev),
                     torch.empty(m, dtype=torch.int32, device=dev) if plan.path_tracing else None,
                     torch.empty(m, dtype=torch.uint8, device=dev) if plan.group_octants else None, m)

    def _level_fused(self, plan, q, level, last):
        """One level as ONE launch of mr_trace_level; returns (rays, shadow rays) and the next queue (None after the last)."""
        sc, n = self.scene, q.n
        order = None
        if q.octs is not None:                          # grouped waves share a direction sign: the default control flow
            order = torch.empty(n, dtype=torch.int32, device=self.device)
            sc.order_by_octant(q.rays, n, order, d_octants=q.octs, stream=plan.stream)
        cnts = torch.zeros(3, dtype=torch.int64, device=self.device)        # rays, shadow rays, children
        out = NO_QUEUE if last else self._children(plan, n)
        children = binding.MR_LEVEL_LAST if last else (binding.MR_LEVEL_PATH if plan.path_tracing else binding.MR_LEVEL_SPECULAR)
        sc.trace_level(q.rays, q.weights, q.pixels, q.ids, n, self.d_slots, self.desc["light"], self.desc["wattage"],
                       children=children, d_out_rays=out.rays, d_out_weights=out.weights, d_out_pixels=out.pixels, d_out_ids=out.ids,
                       d_out_count=None if last else cnts[2:], d_counts=cnts[:2], spp=self.spp,
                       flags=plan.level_flags(level, order is not None)[2], seed=plan.path_seed, bounce=level, kinds=plan.path_kinds,
                       stream=plan.stream, d_out_octants=out.octs, d_order=order)
        host = cnts.tolist()
        return (n, host[1]), None if last else out.first(host[2])

    def _level_buffers(self, plan, n, level, last):
        """What a one-launch light-list level of n rays (or samples) writes besides pixels: hit records, and bumped normals on a
        procedural scene, with photon maps only; the call's five counters and the children's; the children's queue (NO_QUEUE
        after the last level), under path tracing with an environment with their low-res bytes."""
        f32 = dict(dtype=torch.float32, device=self.device)
        hits = normal = None
        if plan.photon_maps is not None:                # the photon term reads the level's hit records (and bumped normals)
            hits = self.d_hits if level == 0 else torch.empty((n, 4), **f32)
            normal = torch.empty((n, 3), **f32) if plan.surface else None
        cnts = torch.zeros(6, dtype=torch.int64, device=self.device)
        out = NO_QUEUE if last else self._children(plan, n)
        if plan.path_tracing and not last and plan.environment:
            out = out._replace(low=torch.empty(out.n, dtype=torch.uint8, device=self.device))
        return hits, normal, cnts, out

    def _gather(self, plan, q, hits, normal, rgb):
        """The photon-map term of a level, where the plan has maps: mr_gather_level on the level's queue and hit records"""
        if plan.photon_maps is not None:
            scratch = torch.empty(12 * q.n, dtype=torch.float32, device=self.device)
            self.scene.gather_level(plan.photon_maps[0], plan.photon_maps[1], q.rays, hits, q.n, scratch, rgb, d_normal=normal,
                                    d_weights=q.weights, d_pixels=q.pixels, max_dist=plan.max_dist, nphotons=plan.nphotons,
                                    spp=self.spp, stream=plan.stream)

    def _level_lights(self, plan, q, level, last, rgb=None):
        """One level as ONE launch of mr_trace_level_lights or, under path tracing, of mr_trace_level_lights_path (then
        mr_gather_level, with photon maps); returns (rays, shadow rays) and the next queue (None after the last).  rgb: the
        pixels the level adds to (None: d_slots)."""
        rgb = self.d_slots if rgb is None else rgb
        hits, normal, cnts, out = self._level_buffers(plan, q.n, level, last)
        common = dict(environment=plan.environment, d_hits=hits, d_normal=normal, d_out_rays=out.rays, d_out_weights=out.weights,
                      d_out_pixels=out.pixels, d_out_count=None if last else cnts[5:], d_counts=cnts[:5], spp=self.spp,
                      flags=plan.level_flags(level)[2], stream=plan.stream)
        if plan.path_tracing:
            self.scene.trace_level_lights_path(q.rays, q.weights, q.pixels, q.ids, q.n, rgb,
                                               children=binding.MR_LEVEL_LAST if last else binding.MR_LEVEL_PATH, d_out_ids=out.ids,
                                               seed=plan.path_seed, bounce=level, kinds=plan.path_kinds, d_lowres=q.low,
                                               d_out_lowres=out.low, **common)
        else:
            self.scene.trace_level_lights(q.rays, q.weights, q.pixels, q.n, rgb,
                                          children=binding.MR_LEVEL_LAST if last else binding.MR_LEVEL_SPECULAR, **common)
        self._gather(plan, q, hits, normal, rgb)
        host = cnts.tolist()
        return (q.n, host[1]), None if last else out.first(host[5])

    def _frame_levels(self, plan, depth):
        """The "frame" driver: level 0 as _frame_level0, the further levels as _level_lights on its
        children, adding into d_rgb; returns (rays, shadow rays) per level."""
        if self.n == 0 or depth < 0:
            return []
        counts, queue = self._frame_level0(plan, depth == 0)
        per_level = [counts]
        for level in range(1, depth + 1):
            if queue.n == 0:
                break
            counts, queue = self._level_lights(plan, queue, level, level == depth, rgb=self.d_rgb)
            per_level.append(counts)
        return per_level

    def _eye_call(self, plan, name):
        """A Scene call that makes level 0's eye rays for the renderer's one window, as (method, lens, keywords).  The pinhole or
        lens choice: Scene's method `name` and lens = (), or on a lens route its _lens twin and lens = (aperture, focus plane).
        The keywords: the window, the sampling and the plan's, which every such call takes."""
        (y0, y1), = self.bands
        common = dict(y0=y0, y1=y1, spp=self.spp, jitter=self.jitter, seed=self.seed, tiled=self.tiled, flags=plan.level_flags(0)[2],
                      stream=plan.stream, environment=plan.environment, kinds=plan.path_kinds, path_seed=plan.path_seed)
        if plan.lens is None:
            return getattr(self.scene, name), (), common
        return getattr(self.scene, name + "_lens"), (plan.lens["aperture"], plan.lens["focus_plane"]), common

    def _device_levels(self, plan, depth, queue_capacity, samples=None):
        """The "device" driver: ONE mr_render_recursion, or on a route with photons ONE mr_render_recursion_photons with the plan's
        maps, each through the thin lens on a lens route (_eye_call).  Then ONE read of the counters; returns (rays, shadow rays)
        per level, cut at the first level without rays; RuntimeError if a level was truncated.
        samples: the frame's samples per pixel -- ONE mr_render_recursion[_photons]_passes instead (_device_passes)."""
        if self.n == 0 or depth < 0:
            return []
        if samples is not None:
            return self._device_passes(plan, depth, queue_capacity, int(samples))
        photons = plan.route.photons
        cap = plan.fan * self.n if queue_capacity is None else int(queue_capacity)
        children = binding.MR_LEVEL_PATH if plan.path_tracing else binding.MR_LEVEL_SPECULAR
        recursion, lens, common = self._eye_call(plan, "render_recursion_photons" if photons else "render_recursion")
        if photons:
            need = self.scene.recursion_photons_workspace_bytes(self.cam, self.W, self.H, depth, cap, y0=common["y0"], y1=common["y1"],
                                                                spp=self.spp, children=children, environment=plan.environment,
                                                                kinds=plan.path_kinds)
        else:
            need = self.scene.recursion_workspace_bytes(depth, cap, children=children, environment=plan.environment,
                                                        kinds=plan.path_kinds)
        if self.d_recursion is None or self.d_recursion.numel() < need:
            self.d_recursion = torch.empty(max(need, 16), dtype=torch.uint8, device=self.device)
        if self.d_level_counts is None or self.d_level_counts.shape[0] < depth + 1:
            self.d_level_counts = torch.zeros((depth + 1, 8), dtype=torch.int64, device=self.device)
        # the recursions take the lens by keyword
        common.update(zip(("aperture", "focus_plane"), lens), queue_capacity=cap, children=children, workspace_bytes=need)
        if photons:
            recursion(self.cam, self.W, self.H, self.d_rgb, self.d_level_counts, depth, plan.photon_maps[0], plan.photon_maps[1],
                      self.d_recursion, max_dist=plan.max_dist, nphotons=plan.nphotons, **common)
        else:
            recursion(self.cam, self.W, self.H, self.d_rgb, self.d_level_counts, depth, d_workspace=self.d_recursion if depth > 0 else None,
                      **common)
        host = self.d_level_counts[:depth + 1].tolist()             # the one read-back of the frame
        per_level = []
        for level, row in enumerate(host):
            if row[0] == 0:
                break
            per_level.append((row[0], row[1]))
            if level < depth and row[5] > cap:
                raise RuntimeError("render_specular: level %d emitted %d children, queue_capacity is %d: the frame was truncated "
                                   "(%d x the samples always suffice)" % (level, row[5], cap, plan.fan ** depth))
        return per_level

    def _device_passes(self, plan, depth, queue_capacity, samples):
        """_device_levels for a frame of `samples` samples per pixel in passes of the renderer's spp: the workspace of ONE pass, the
        counters of every pass, one call, one read-back; per_level summed over the passes."""
        photons = plan.route.photons
        cap = plan.fan * self.n if queue_capacity is None else int(queue_capacity)
        children = binding.MR_LEVEL_PATH if plan.path_tracing else binding.MR_LEVEL_SPECULAR
        _, _, common = self._eye_call(plan, "render_recursion")
        if photons:
            need = self.scene.recursion_photons_workspace_bytes(self.cam, self.W, self.H, depth, cap, y0=common["y0"], y1=common["y1"],
                                                                spp=self.spp, children=children, environment=plan.environment,
                                                                kinds=plan.path_kinds)
        else:
            need = self.scene.recursion_workspace_bytes(depth, cap, children=children, environment=plan.environment,
                                                        kinds=plan.path_kinds)
        n_passes = len(binding.passes_plan(self.spp, samples))
        if self.d_recursion is None or self.d_recursion.numel() < need:
            self.d_recursion = torch.empty(max(need, 16), dtype=torch.uint8, device=self.device)
        if self.d_pass_counts is None or self.d_pass_counts.shape[0] < n_passes or self.d_pass_counts.shape[1] != depth + 1:
            self.d_pass_counts = torch.zeros((n_passes, depth + 1, 8), dtype=torch.int64, device=self.device)
        common.update(lens=plan.lens, queue_capacity=cap, children=children, workspace_bytes=need)
        if photons:
            self.scene.render_recursion_photons_passes(self.cam, self.W, self.H, self.d_rgb, self.d_pass_counts, depth, samples,
                                                       plan.photon_maps[0], plan.photon_maps[1], self.d_recursion,
                                                       max_dist=plan.max_dist, nphotons=plan.nphotons, **common)
        else:
            self.scene.render_recursion_passes(self.cam, self.W, self.H, self.d_rgb, self.d_pass_counts, depth, samples,
                                               d_workspace=self.d_recursion if depth > 0 else None, **common)
        host = self.d_pass_counts[:n_passes].tolist()               # the one read-back of the frame
        total = [[0, 0] for _ in range(depth + 1)]
        for index, block in enumerate(host):
            for level, row in enumerate(block):
                total[level][0] += row[0]
                total[level][1] += row[1]
                if level < depth and row[5] > cap:
                    raise RuntimeError("render_specular: pass %d, level %d emitted %d children, queue_capacity is %d: the frame was "
                                       "truncated (%d x a pass's samples always suffice)" % (index, level, row[5], cap, plan.fan ** depth))
        per_level = []
        for rays, shadow in total:
            if rays == 0:
                break
            per_level.append((rays, shadow))
        return per_level

    def finish(self, d_minmax=None, stream=None):
        """mr_finish_image on d_rgb (Scene.cpp:150-163, 184-197; Image.cpp:47-52): the image's maximum over its non-NaN channel
        values in place of every NaN channel, then the tone map.  Returns the bytes, a uint8 tensor [n_pixels, 3] that the
        renderer keeps."""
        if self.d_bytes is None:
            self.d_bytes = torch.zeros((max(self.n_pixels, 1), 3), dtype=torch.uint8, device=self.device)
        if self.n_pixels:
            self.scene.finish_image(self.d_rgb, self.n_pixels, self.d_bytes, d_minmax=d_minmax, stream=stream)
        return self.d_bytes

    def _frame_level0(self, plan, last):
        """Level 0 as ONE mr_render_level_lights[_lens] straight into d_rgb (then mr_gather_level, with photon maps, on generate()'s
        rays); returns (rays, shadow rays) from the launch's counters and the queue of level 1 (None after the last)."""
        if plan.photon_maps is not None:                # the photon term reads level 0's rays
            self.generate(plan.stream)
        hits, normal, cnts, out = self._level_buffers(plan, self.n, 0, last)
        children = binding.MR_LEVEL_LAST if last else binding.MR_LEVEL_PATH if plan.path_tracing else binding.MR_LEVEL_SPECULAR
        render, lens, common = self._eye_call(plan, "render_level_lights")
        render(self.cam, self.W, self.H, self.d_rgb, *lens, d_hits=hits, d_sample_normal=normal, d_counts=cnts[:5], children=children,
               d_out_rays=out.rays, d_out_weights=out.weights, d_out_pixels=out.pixels, d_out_ids=out.ids,
               d_out_count=None if last else cnts[5:], d_out_lowres=out.low, **common)
        self._gather(plan, Queue(self.d_rays, None, None, None, None, self.n), hits, normal, self.d_rgb)
        host = cnts.tolist()
        return (host[0], host[1]), None if last else out.first(host[5])

    def _level_batched(self, plan, q, level, last):
        """One level as separate launches: trace, environment, surface pass, shade, photon term, children -- whichever of
        them the plan asks for; returns (rays, shadow rays) and the next queue (None after the last)."""
        sc, n, stream = self.scene, q.n, plan.stream
        f32 = dict(dtype=torch.float32, device=self.device)
        hits = self.d_hits if plan.lights and level == 0 else torch.empty((n, 4), **f32)
        trace_flags, _, grouped_flags = plan.level_flags(level, q.octs is not None)
        if q.octs is not None:
            order = torch.empty(n, dtype=torch.int32, device=self.device)
            sc.trace_grouped(q.rays, n, hits, order, grouped_flags, d_octants=q.octs, stream=stream)
        else:
            sc.trace_device(q.rays, n, hits, trace_flags, stream=stream)
        if plan.environment:
            sc.shade_environment(q.rays, hits, n, self.d_slots, d_weights=q.weights, d_pixels=q.pixels, spp=self.spp,
                                 flags=plan.env_lowres if level > 0 else 0, stream=stream)
        color = normal = None
        if plan.surface_pass(last):
            color, normal = torch.empty((n, 3), **f32), torch.empty((n, 3), **f32)
            sc.hit_surface(q.rays, hits, n, color, normal, stream=stream)
        cnt = torch.zeros(1, dtype=torch.int64, device=self.device)
        self._shade(plan, q, hits, color, normal, cnt, level)
        self._gather(plan, q, hits, normal if plan.surface else None, self.d_slots)
        counts = (n, int(cnt.item()))
        return counts, None if last else self._generate(plan, q, hits, color, normal, level)

    def _shade(self, plan, q, hits, color, normal, cnt, level):
        """A batched level's direct light, weight x Phong::shade added to the ray's pixel: the scene's light list in one launch,
        or the description's point light through a shadow batch; then the renderer's square lights.  Each from the surface
        pass's colour and normal where the plan says so.  cnt[0]: the level's shadow rays."""
        sc, n, stream = self.scene, q.n, plan.stream
        L, W = self.desc["light"], self.desc["wattage"]
        trace_flags, shade_flags, _ = plan.level_flags(level)
        if plan.lights:
            if plan.surface:
                sc.shade_lights_surface(q.rays, hits, color, normal, n, self.d_slots, d_weights=q.weights, d_pixels=q.pixels,
                                        spp=self.spp, flags=shade_flags, d_counts=cnt, stream=stream)
            else:
                sc.shade_lights(q.rays, hits, n, self.d_slots, d_weights=q.weights, d_pixels=q.pixels, spp=self.spp,
                                flags=shade_flags, d_counts=cnt, stream=stream)
        else:
            f32 = dict(dtype=torch.float32, device=self.device)
            sh_rays, sh_hits = torch.empty((n, 8), **f32), torch.empty((n, 4), **f32)
            src = torch.empty(n, dtype=torch.int32, device=self.device)
            sc.gen_shadow_rays(q.rays, hits, n, L, sh_rays, src, cnt, stream=stream)
            sc.trace_indirect(sh_rays, cnt, n, sh_hits, trace_flags, stream=stream)         # closest hit: the occluder matters
            if plan.surface:
                sc.shade_accumulate_surface(q.rays, hits, color, normal, q.weights, q.pixels, n, sh_rays, sh_hits, src, cnt, L, W,
                                            self.d_slots, spp=self.spp, stream=stream)
            else:
                sc.shade_accumulate(q.rays, hits, q.weights, q.pixels, n, sh_rays, sh_hits, src, cnt, L, W, self.d_slots,
                                    spp=self.spp, stream=stream)
        if plan.square == "surface":
            sc.shade_square_lights_surface(plan.square_lights, self.square_samples, q.rays, hits, color, normal, n, self.d_slots,
                                           seed=self.seed + level, d_weights=q.weights, d_pixels=q.pixels, spp=self.spp,
                                           flags=shade_flags, d_counts=cnt, stream=stream)
        elif plan.square == "plain":
            sc.shade_square_lights(plan.square_lights, self.square_samples, q.rays, hits, n, self.d_slots, seed=self.seed + level,
                                   d_weights=q.weights, d_pixels=q.pixels, spp=self.spp, flags=shade_flags, d_counts=cnt,
                                   stream=stream)

    def _generate(self, plan, q, hits, color, normal, level):
        """The next level's queue by ballot compaction: the path-tracing generators (from the surface buffers where the plan
        says so) or the reflect / Fresnel / refract children (about the surface pass's normal on a scene with bumped_specular,
        which is procedural, so every level has run the pass)."""
        sc, n = self.scene, q.n
        out = self._children(plan, n)
        cnt = torch.zeros(1, dtype=torch.int64, device=self.device)
        if not plan.path_tracing and sc.bumped_specular is True:      # a reflective STONE material: N from the surface pass
            sc.gen_secondary_rays_surface(q.rays, hits, normal, q.weights, q.pixels, n, out.rays, out.weights, out.pixels, cnt,
                                          spp=self.spp, stream=plan.stream, d_out_octants=out.octs)
        elif not plan.path_tracing:
            sc.gen_secondary_rays(q.rays, hits, q.weights, q.pixels, n, out.rays, out.weights, out.pixels, cnt, spp=self.spp,
                                  stream=plan.stream, d_out_octants=out.octs)
        elif plan.surface_children:
            sc.gen_path_rays_surface(q.rays, hits, color, normal, q.weights, q.pixels, q.ids, n, out.rays, out.weights, out.pixels,
                                     out.ids, cnt, spp=self.spp, seed=plan.path_seed, bounce=level, kinds=plan.path_kinds,
                                     stream=plan.stream, d_out_octants=out.octs)
        else:
            sc.gen_path_rays(q.rays, hits, q.weights, q.pixels, q.ids, n, out.rays, out.weights, out.pixels, out.ids, cnt,
                             spp=self.spp, seed=plan.path_seed, bounce=level, kinds=plan.path_kinds, stream=plan.stream,
                             d_out_octants=out.octs)
        return out.first(int(cnt.item()))

    def ray_counts(self):
        """(primary, shadow) of the last step -- synchronises the whole device (the step may have run on any stream)."""
        if not self.n:
            return 0, 0
        torch.cuda.synchronize(self.device)
        return self.n, int(self.d_count.item())
