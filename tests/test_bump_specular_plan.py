"""Reflective bump-mapped materials without a GPU (include/miro_hip_bump.h, csrc/mr_bump_surface.hip, csrc/mr_level_lights_bump.hip,
csrc/mr_level_lights_queued_bump.hip): the one new symbol and its list, the older lists as they were, the polished room's material
table, the three new units' kernels against their records, what FrameRenderer launches on such a scene, and the float32 restatement
of Ray::reflect (Ray.h:143-163) that tests/test_bump_specular.py holds the device to, checked here against a float64 evaluation of
the same lines."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kernel_budget  # noqa: E402

F = np.float32
NAME = "mr_gen_secondary_rays_surface"
OLDER = ("miro_hip.h", "miro_hip_surface.h", "miro_hip_frame.h", "miro_hip_render.h", "miro_hip_recursion.h",
         "miro_hip_recursion_photons.h", "miro_hip_lens.h", "miro_hip_passes.h")
VARIANTS = (1818, 826, 267, 43, 88, 73)                 # kTraceExact, ExactObj, Product, ProductObj, Vote, VoteProduct
EPSILON = F(1e-4)                                       # Miro.h:9
RTOL, ATOL_OF_MAX = 1e-5, 1e-7                          # tests/test_procedural.py:29, the bound of its float32 restatements


# ---- the restatement: Ray.h:143-163 without PATH_TRACING, in rec::ChildGen's operation order -------------------------------
def restate_reflect(d, N, P, dtype=F):
    """Ray::reflect.  d_r = d - 2 dot(N, d) N (Ray.h:160), normalize (:161), Ray(P + d_r * epsilon, d_r) (:162), every operation
    rounded to `dtype`: the dot product summed as (x + y) + z, the length likewise, one reciprocal of the square root times each
    component.  Rows of d, N, P; returns (origin, direction)."""
    d, N, P = (np.asarray(a, dtype) for a in (d, N, P))
    two = dtype(2) * ((N[:, 0] * d[:, 0] + N[:, 1] * d[:, 1]) + N[:, 2] * d[:, 2])
    r = d - two[:, None] * N
    inv = dtype(1) / np.sqrt((r[:, 0] * r[:, 0] + r[:, 1] * r[:, 1]) + r[:, 2] * r[:, 2])
    r = r * inv[:, None]
    return P + r * dtype(EPSILON), r


def within(got, want):
    """the bound tests/test_procedural.py holds a float32 restatement to: RTOL x |want| + ATOL_OF_MAX x max |want|"""
    want = np.asarray(want, np.float64)
    err = np.abs(np.asarray(got, np.float64) - want)
    return err, bool((err <= RTOL * np.abs(want) + ATOL_OF_MAX * np.abs(want).max()).all())


def unit_rows(rng, n):
    v = rng.standard_normal((n, 3))
    return (v / np.linalg.norm(v, axis=1)[:, None]).astype(F)


U32 = 2.0 ** -24                                        # the unit roundoff of float32


def test_float32_restatement_of_ray_reflect_against_float64():
    """10 000 random unit d and N (a float32 unit vector is unit to a few 1e-8), P in the room's range: origin and direction of the
    float32 evaluation against the float64 evaluation of the same lines on the same inputs.  The bound comes from the format, not
    from the result: a component of d_r before normalize carries the dot product's error (three products and two sums of terms
    whose magnitudes sum to at most 1: 2.5 U32, doubled, times |N_c| <= 1: 5 U32), the rounding of 2 dot * N_c (at most 2: U32)
    and of the subtraction (at most 3: 1.5 U32); normalize adds the squared length's three products and two sums, the square
    root, the reciprocal and the product, about 4 U32 relative on a component of at most 1.  12 U32 in all on the direction; the
    origin is P + d_r * epsilon, whose one rounding at |P| <= 4 is at most U32 x 4 and whose second term is 1e-4 of the
    direction's error: inside 12 U32 x max |origin|.  Both stay inside their bound, and the mirror law holds in float64
    (dot(r, N) = -dot(d, N), |r| = 1)."""
    rng = np.random.default_rng(168)
    d, N = unit_rows(rng, 10000), unit_rows(rng, 10000)
    P = rng.uniform(-4, 4, (10000, 3)).astype(F)
    o32, r32 = restate_reflect(d, N, P)
    o64, r64 = restate_reflect(d, N, P, np.float64)
    assert o32.dtype == F and r32.dtype == F and o64.dtype == np.float64
    for what, got, want in (("direction", r32, r64), ("origin", o32, o64)):
        err = np.abs(got.astype(np.float64) - want).max()
        bound = 12 * U32 * max(1.0, np.abs(want).max())
        print("%s: largest deviation %.3g, bound %.3g" % (what, err, bound))
        assert err <= bound, (what, err, bound)
    dn = (d.astype(np.float64) * N).sum(axis=1)
    assert np.abs((r64 * N).sum(axis=1) + dn).max() < 1e-6 and np.abs(np.linalg.norm(r64, axis=1) - 1).max() < 1e-12
    flat = np.tile(F([0, 1, 0]), (10000, 1))            # about another normal the direction is another one, by far more than any bound
    assert np.abs(restate_reflect(d, flat, P)[1] - r32).max() > 0.5


# ---- the symbol and the lists ------------------------------------------------------------------------------------------------
def header(name):
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", name)).read(), flags=re.S)


def test_the_symbol_is_exported_declared_and_bound(miro):
    """Fails on the parent commit: the symbol, the header and the ninth list are this feature's.  The eight older lists are as
    they were, and miro_hip.h alone reaches the new header (through miro_hip_passes.h, below its declarations)."""
    from miro_amd import binding
    declared = lambda h, name: re.search(r"\bmr_status\s+%s\s*\(" % name, header(h)) is not None            # noqa: E731
    assert re.findall(r"\bmr_status\s+(\w+)\s*\(", header("miro_hip_bump.h")) == [NAME]
    assert binding.BUMP_SYMBOLS == [NAME]
    assert hasattr(miro.lib(), NAME) and getattr(miro.lib(), NAME).restype is C.c_int32
    assert not any(declared(h, NAME) for h in OLDER)
    older = [miro.EXPORTED_SYMBOLS, binding.SURFACE_SYMBOLS, binding.FRAME_SYMBOLS, binding.RENDER_SYMBOLS, binding.RECURSION_SYMBOLS,
             binding.RECURSION_PHOTONS_SYMBOLS, binding.LENS_SYMBOLS, binding.PASSES_SYMBOLS]
    assert [len(names) for names in older] == [69, 9, 3, 1, 2, 2, 3, 4]
    assert all(NAME not in names and len(set(names)) == len(names) for names in older)
    assert binding.PASSES_SYMBOLS == ["mr_render_passes_plan", "mr_render_recursion_passes", "mr_render_recursion_photons_passes", "mr_finish_image"]
    assert binding.LENS_SYMBOLS == ["mr_render_level_lights_lens", "mr_render_recursion_lens", "mr_render_recursion_photons_lens"]
    assert binding.RECURSION_PHOTONS_SYMBOLS == ["mr_render_recursion_photons_workspace", "mr_render_recursion_photons"]
    assert binding.RECURSION_SYMBOLS == ["mr_render_recursion_workspace", "mr_render_recursion"]
    assert binding.RENDER_SYMBOLS == ["mr_render_level_lights"]
    assert binding.FRAME_SYMBOLS == ["mr_render_lights_environment", "mr_trace_level_lights", "mr_trace_level_lights_path"]
    assert "mr_gen_secondary_rays" in miro.EXPORTED_SYMBOLS and "mr_gen_path_rays_surface" in binding.SURFACE_SYMBOLS
    raw = lambda h: open(os.path.join(ROOT, "include", h)).read().rstrip()                                  # noqa: E731
    assert raw("miro_hip_passes.h").endswith('#include "miro_hip_bump.h"\n#endif /* MIRO_HIP_PASSES_H */')
    assert raw("miro_hip_bump.h").endswith("#endif /* MIRO_HIP_BUMP_H */")
    # mr_gen_secondary_rays with d_normal after d_hits, argument for argument
    plain, surf = miro.lib().mr_gen_secondary_rays.argtypes, getattr(miro.lib(), NAME).argtypes
    assert list(surf) == list(plain[:3]) + [C.c_void_p] + list(plain[3:])
    assert hasattr(miro.Scene, "gen_secondary_rays_surface") and isinstance(miro.Scene.bumped_specular, property)
    assert miro.Scene.bumped_specular.fset is None


def test_the_rule_on_a_host_only_scene(miro):
    """mr_scene_set_textures from its arguments and the material table alone: ks != 0 on a STONE material is accepted (where
    the texture says MR_TEX_REFLECTIVE, as the binding's dict(stone=...) does) and remembered, kt != 0 is MR_ERR_INVALID with a message that names transmission's reason, and a refused table leaves the
    flag alone.  Fails on the parent commit."""
    from miro_amd import binding
    s = miro.Scene()
    s.add_triangle([0, 0, 0, 1, 0, 0, 0, 1, 0], [0, 0, 1] * 3)
    s.build(4, host_only=True)
    white, zero = (1.0, 1.0, 1.0), (0.0, 0.0, 0.0)
    s.set_materials([(white, zero, zero, 20.0, 1.0), (white, (0.3, 0.3, 0.3), zero, 20.0, 1.0), (white, zero, (0.0, 0.1, 0.0), 20.0, 1.5)], [0])
    assert s.bumped_specular is False
    s.set_textures([dict(stone=3.0)], [0, binding.MR_NO_TEXTURE, binding.MR_NO_TEXTURE])
    assert s.bumped_specular is False and s.procedural
    s.set_textures([dict(stone=3.0), dict(stem=2.0)], [binding.MR_NO_TEXTURE, 1, binding.MR_NO_TEXTURE])      # a STEM bumps nothing
    assert s.bumped_specular is False
    s.set_textures([dict(stone=3.0)], [0, 0, binding.MR_NO_TEXTURE])
    assert s.bumped_specular is True
    with pytest.raises(miro.MiroError) as e:
        s.set_textures([dict(stone=3.0)], [0, 0, 0])
    msg = str(e.value)
    assert e.value.status == binding.MR_ERR_INVALID and "kt" in msg and "occluder" in msg and "Phong.cpp:99-113" in msg
    assert s.bumped_specular is True                     # the earlier table stands
    # the descriptor's word: MR_TEX_REFLECTIVE in reserved[0] of a STONE texture, which Scene.set_textures sets for dict(stone=...).
    # Without it the table is refused as it always was; no other kind and no other reserved word may carry it
    assert binding.MR_TEX_REFLECTIVE == 1
    with pytest.raises(miro.MiroError) as e:
        s.set_textures([dict(stone=3.0, reflective=False)], [0, 0, binding.MR_NO_TEXTURE])
    assert e.value.status == binding.MR_ERR_INVALID and "STONE" in str(e.value) and "MR_TEX_REFLECTIVE" in str(e.value)
    assert s.bumped_specular is True
    s.set_textures([dict(stone=3.0, reflective=False)], [0, binding.MR_NO_TEXTURE, binding.MR_NO_TEXTURE])   # diffuse only: no flag needed
    assert s.bumped_specular is False
    L = miro.lib()

    def raw(kind, word, value, mt):
        d = binding.TextureDesc()
        d.kind, d.scale = kind, 3.0
        d.reserved[word] = value
        return L.mr_scene_set_textures(s.h, (binding.TextureDesc * 1)(d), 1, binding._u32p(np.array(mt, np.uint32)))

    none = binding.MR_NO_TEXTURE
    assert raw(binding.MR_TEX_STONE, 0, 1, [0, 0, none]) == binding.MR_OK
    assert raw(binding.MR_TEX_STONE, 0, 1, [0, none, 0]) == binding.MR_ERR_INVALID and b"kt" in L.mr_last_error()
    assert raw(binding.MR_TEX_STONE, 0, 0, [none, 0, none]) == binding.MR_ERR_INVALID and b"MR_TEX_REFLECTIVE" in L.mr_last_error()
    for kind, word, value in ((binding.MR_TEX_STONE, 0, 2), (binding.MR_TEX_STONE, 1, 1), (binding.MR_TEX_STEM, 0, 1), (binding.MR_TEX_CHECKER, 0, 1)):
        assert raw(kind, word, value, [0, none, none]) == binding.MR_ERR_INVALID and b"reserved" in L.mr_last_error(), (kind, word, value)
    s.set_textures([])
    assert s.bumped_specular is False and not s.procedural


def test_the_polished_room():
    """photon_room_stone() with the floor material (kd 1, ks 0.3, kt 0, shininess 20, index 1) and the STONE wall x = -2 on a
    material of its own with ks 0.1; everything else is that room's"""
    from miro_amd import scenes
    stone, pol = scenes.photon_room_stone(), scenes.photon_room_polished()
    one, zero = (1.0, 1.0, 1.0), (0.0, 0.0, 0.0)
    assert pol["materials"][0] == (one, (0.3, 0.3, 0.3), zero, 20.0, 1.0)
    assert pol["objects"][-1][0] == "plane" and pol["objects"][-1][3] == 0                       # the floor plane: material 0
    wall = pol["materials"][pol["prim_material"][0]]
    assert pol["prim_material"][:2] == [5, 5] and wall[0] == one and wall[1] == (0.1, 0.1, 0.1) and wall[2] == zero
    assert pol["materials"][1:5] == stone["materials"][1:] and pol["prim_material"][2:] == stone["prim_material"][2:]
    assert pol["textures"] == stone["textures"] == [dict(stone=3.0), dict(stone=20.0)]
    assert pol["material_texture"] == stone["material_texture"] + [1]
    assert pol["objects"] == stone["objects"] and np.array_equal(pol["tidx"], stone["tidx"])
    assert all(m[2] == zero for m, t in zip(pol["materials"], pol["material_texture"]) if t != 0xFFFFFFFF)   # no STONE material transmits


# ---- the kernels ---------------------------------------------------------------------------------------------------------------
def test_the_new_kernels_stay_inside_the_verified_envelope():
    """The three new units, each against its own record (written from the build whose GPU run of tests/test_bump_specular.py was
    green) AND the worst value among the kernels of tests/golden/kernel_budget.json: no dynamic stack, no more spilled VGPRs, no
    more scratch per lane, no fewer waves.  Six BUMPED level kernels per unit, one per traversal variant, at four waves per SIMD
    or more; one generator kernel without scratch."""
    gen = kernel_budget.unit_kernels("mr_bump_surface")
    assert len(gen) == 1 and all("children_bump_kernel" in k for k in gen)
    assert all(v["scratch_bytes_per_lane"] == 0 and v["vgprs_spilled"] == 0 for v in gen.values())
    kernel_budget.assert_inside_envelope(gen, "kernel_budget_bump_surface.json", also_main=True)
    for unit, kernel in (("mr_level_lights_bump", "level_lights_bumped_kernel"), ("mr_level_lights_queued_bump", "level_lights_queued_bumped_kernel")):
        cur = kernel_budget.unit_kernels(unit)
        assert len(cur) == len(VARIANTS)
        for var in VARIANTS:
            assert sum("%sILi%dEE" % (kernel, var) in k for k in cur) == 1, (unit, var)
        assert not any(v["dynamic_stack"] for v in cur.values()) and all(v["waves_per_simd"] >= 4 for v in cur.values())
        kernel_budget.assert_inside_envelope(cur, "kernel_budget_%s.json" % unit.replace("mr_", "", 1), also_main=True)


# ---- the driver ----------------------------------------------------------------------------------------------------------------
def test_the_batched_driver_calls_the_surface_generator_on_a_bumped_scene_only():
    """FrameRenderer on the recording scene of tests/test_frame_plan.py (a procedural table): with bumped_specular the specular
    levels' children come from gen_secondary_rays_surface, fed the level's own normal buffer, and every other call is what it was;
    without it (the stand-in answers every unknown name with a method, which is not True) gen_secondary_rays is called as before.
    With path_tracing an explicit surface_children=False raises and None turns into gen_path_rays_surface."""
    torch = pytest.importorskip("torch")
    from miro_amd import frame
    from test_frame_plan import DESC, H, SPP, W, RecordingScene

    class Bumped(RecordingScene):
        bumped_specular = True

        def launch(self, name, a, kw):
            if name == "gen_secondary_rays_surface":                      # (rays, hits, normal, weights, pixels, n, out x 3, count)
                a[9][0] = self.part(a[5], self.child)
                return None
            return super().launch(name, a, kw)

    def run(cls, **kw):
        sc = cls(2, True, (3, 4), (1, 2), False)
        fr = frame.FrameRenderer(sc, DESC, W, H, spp=SPP, device=torch.device("cpu"))
        return sc, fr, fr.render_specular(**kw)

    plain, _, levels_plain = run(RecordingScene, depth=2)
    bumped, _, levels_bumped = run(Bumped, depth=2)
    names = lambda sc: [c[0] for c in sc.calls]                                                               # noqa: E731
    assert levels_plain == levels_bumped and len(levels_plain) == 3
    assert "gen_secondary_rays_surface" not in names(plain) and names(plain).count("gen_secondary_rays") == 2
    assert "gen_secondary_rays" not in names(bumped) and names(bumped).count("gen_secondary_rays_surface") == 2
    assert [n.replace("_rays_surface", "_rays") if n.startswith("gen_secondary") else n for n in names(bumped)] == names(plain)
    normal = None
    for call in bumped.calls:
        if call[0] == "hit_surface":
            normal = call[1][4]                                           # the level's normal buffer
        if call[0] == "gen_secondary_rays_surface":
            assert normal is not None and call[1][2] == normal and call[1][2][0] == "tensor"
            normal = None                                                 # the next level's generator reads the next level's pass
    sc = Bumped(2, True, (3, 4), (1, 2), False)
    fr = frame.FrameRenderer(sc, DESC, W, H, spp=SPP, device=torch.device("cpu"))
    with pytest.raises(ValueError) as e:
        fr.render_specular(depth=1, path_tracing=True, surface_children=False)
    assert "bumped_specular" in str(e.value) and "surface_children=False" in str(e.value) and sc.calls == []
    fr.render_specular(depth=1, path_tracing=True)
    assert "gen_path_rays_surface" in names(sc) and "gen_path_rays" not in names(sc)
    with pytest.raises(ValueError):                                       # a plain procedural scene keeps its own rule: DIFFUSE only
        run(RecordingScene, depth=1, path_tracing=True, surface_children=False, path_kinds=7)
    run(RecordingScene, depth=1, path_tracing=True, surface_children=False, path_kinds=3)
