"""The statuses and mr_last_error() texts of the four recursion entry points -- mr_render_recursion_workspace, mr_render_recursion,
mr_render_recursion_photons_workspace, mr_render_recursion_photons -- against tests/golden/recursion_errors.json, without a GPU.

The fixture was recorded from the library of the commit BEFORE the two entry points were put on one driver and one preamble
(`MIRO_LIB=<that build's libmiro_hip.so> python tests/test_recursion_errors.py` writes it), never from the code under test, so the
test also passes on that commit: it does not show a change, it holds the answers from then on -- above all WHICH check answers
first when several things are wrong at once, which the word-in-message assertions of tests/test_recursion_device_plan.py and
tests/test_recursion_photons_plan.py leave open.

The table: every MR_ERR_INVALID and MR_ERR_STATE case of test_argument_errors_come_before_the_scene_and_the_device in those two
files (a host-only one-triangle scene with a light, two unbalanced maps, an unbuilt scene, a scene without lights), each put to
all four entry points -- a workspace query gets the case's two descriptors and ignores the rest --, then the double faults."""
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "recursion_errors.json")
ENTRIES = ["mr_render_recursion_workspace", "mr_render_recursion", "mr_render_recursion_photons_workspace", "mr_render_recursion_photons"]


def variations(binding):
    """(name, frame descriptor or None, recursion descriptor or None, what differs from the good call's arguments).  `bytes` is
    symbolic, since the two render calls need different workspaces: "need" what the case's descriptors ask for, "short" one byte
    less, "specular" what the good call's specular queues ask for, "queues" mr_render_recursion's size, or a number"""
    from test_frame_lights import frame_desc
    from test_recursion_device_plan import PATH, rdesc

    def tiled():
        fd = frame_desc(binding)
        fd.tiled = 1
        return fd

    p = lambda a: C.c_void_p(a)                                                   # noqa: E731
    fd, ok = frame_desc(binding), rdesc()
    depth0 = rdesc(depth=0, children=0, capacity=0)
    v = [
        # both tests' MR_ERR_INVALID lists
        ("null_scene", fd, ok, dict(scene=None)), ("null_frame", None, ok, {}), ("null_rgb", fd, ok, dict(rgb=None)),
        ("empty_image", frame_desc(binding, W=0), ok, {}), ("spp_3", frame_desc(binding, spp=3), ok, {}),
        ("flag_any", frame_desc(binding, flags=binding.MR_TRACE_ANY), ok, {}), ("flag_bit30", frame_desc(binding, flags=1 << 30), ok, {}),
        ("misaligned_rgb", fd, ok, dict(rgb=p(8194))), ("misaligned_counts", fd, ok, dict(counts=p((1 << 16) + 4))),
        ("null_desc", fd, None, {}), ("null_counts", fd, ok, dict(counts=None)),
        ("depth_65", fd, rdesc(depth=65), {}), ("children_0", fd, rdesc(children=0), {}), ("children_7", fd, rdesc(children=7), {}),
        ("environment_2", fd, rdesc(environment=2), {}),
        ("path_kinds_0", fd, rdesc(children=PATH, kinds=0), {}), ("path_kinds_8", fd, rdesc(children=PATH, kinds=8), {}),
        ("reserved_0", fd, rdesc(reserved=0), {}), ("reserved_4", fd, rdesc(reserved=4), {}),
        ("capacity_0", fd, rdesc(capacity=0), {}), ("capacity_2_31", fd, rdesc(capacity=1 << 31), {}),
        ("null_workspace", fd, ok, dict(ws=None)), ("misaligned_workspace", fd, ok, dict(ws=p((1 << 20) + 8))),
        ("depth_0_no_workspace", fd, depth0, dict(ws=None, bytes=0)),
        ("bytes_short", fd, ok, dict(bytes="short")), ("bytes_0", fd, ok, dict(bytes=0)), ("bytes_queues", fd, ok, dict(bytes="queues")),
        ("bytes_specular_for_path", fd, rdesc(children=PATH), dict(bytes="specular")),
        ("both_maps_null", fd, ok, dict(g=None, c=None)),
        ("nphotons_0", fd, ok, dict(k=0)), ("nphotons_513", fd, ok, dict(k=513)),
        ("max_dist_0", fd, ok, dict(dist=0.0)), ("max_dist_negative", fd, ok, dict(dist=-1.0)), ("max_dist_nan", fd, ok, dict(dist=float("nan"))),
        ("tiled", tiled(), ok, {}),
        # both tests' MR_ERR_STATE lists
        ("good", fd, ok, {}), ("good_depth_0", fd, depth0, {}), ("good_depth_64", fd, rdesc(depth=64), {}),
        ("good_global_only", fd, ok, dict(c=None)), ("good_caustic_only_512", fd, ok, dict(g=None, k=512)),
        ("unbuilt", fd, ok, dict(scene="unbuilt")), ("unbuilt_reserved_2", fd, rdesc(reserved=2), dict(scene="unbuilt")),
        ("unbuilt_nphotons_0", fd, ok, dict(scene="unbuilt", k=0)),
        ("no_lights", fd, ok, dict(scene="dark")),
        # two things wrong at once: which check answers
        ("misaligned_rgb+null_counts", fd, ok, dict(rgb=p(8194), counts=None)),
        ("flag_bit30+depth_65", frame_desc(binding, flags=1 << 30), rdesc(depth=65), {}),
        ("reserved_0+null_workspace", fd, rdesc(reserved=0), dict(ws=None)),
        ("tiled+nphotons_0", tiled(), ok, dict(k=0)),
        ("both_maps_null+bytes_0", fd, ok, dict(g=None, c=None, bytes=0)),
        ("capacity_2_31+tiled", tiled(), rdesc(capacity=1 << 31), {}),
        ("children_0_at_depth_0", fd, rdesc(depth=0, children=0), {}),
        ("null_counts+flag_any", frame_desc(binding, flags=binding.MR_TRACE_ANY), ok, dict(counts=None)),
        ("flag_any+null_desc", frame_desc(binding, flags=binding.MR_TRACE_ANY), None, {}),
        ("spp_3+misaligned_rgb", frame_desc(binding, spp=3), ok, dict(rgb=p(8194))),
        ("empty_image+null_counts", frame_desc(binding, W=0), ok, dict(counts=None)),
        ("depth_65+tiled", tiled(), rdesc(depth=65), {}),
        ("tiled+both_maps_null", tiled(), ok, dict(g=None, c=None)),
        ("nphotons_0+max_dist_0", fd, ok, dict(k=0, dist=0.0)),
        ("max_dist_0+null_workspace", fd, ok, dict(dist=0.0, ws=None)),
        ("misaligned_workspace+bytes_0", fd, ok, dict(ws=p((1 << 20) + 8), bytes=0)),
        ("capacity_0+null_workspace", fd, rdesc(capacity=0), dict(ws=None)),
        ("bytes_0+unbuilt", fd, ok, dict(bytes=0, scene="unbuilt")),
        ("unbuilt+no_maps_resident", fd, ok, dict(scene="unbuilt", c=None)),
        ("no_lights+flag_any", frame_desc(binding, flags=binding.MR_TRACE_ANY), ok, dict(scene="dark")),
        ("depth_0_tiled", tiled(), depth0, {}),
    ]
    assert len({name for name, *_ in v}) == len(v)
    return v


def run(miro):
    """every variation put to every entry point: {"<entry>/<variation>": {"status": ..., "message": ...}}; message: mr_last_error()
    of a refused call, "" for MR_OK"""
    from miro_amd import binding
    from test_frame_lights import frame_desc
    from test_recursion_device_plan import rdesc, workspace as queues
    from test_recursion_photons_plan import workspace as photons_workspace

    L = miro.lib()

    def one_triangle(lights, build):
        s = miro.Scene()
        s.add_triangle([0, 0, 0, 1, 0, 0, 0, 1, 0], [0, 0, 1] * 3)
        if lights:
            s.set_lights([dict(position=(0, 1, 0), wattage=5.0)])
        if build:
            s.build(4, host_only=True)
        return s

    scenes = {"host": one_triangle(True, True), "unbuilt": one_triangle(False, False), "dark": one_triangle(False, True)}
    g, c = miro.PhotonMap(64), miro.PhotonMap(64)
    p = lambda a: C.c_void_p(a)                                                   # noqa: E731
    base = dict(scene="host", g=g.h, c=c.h, dist=1e10, k=50, rgb=p(8192), ws=p(1 << 20), bytes="need", counts=p(1 << 16))

    def need(photons, fd, rd, which):
        """the workspace of the case's descriptors, as the two formula tests spell it; of the good call's where they say nothing"""
        if which == "queues":
            return queues(100, False, 0)
        depth, cap = (rd.depth, rd.queue_capacity_lo) if rd is not None else (3, 100)
        path, env = (rd.children == binding.MR_LEVEL_PATH, rd.environment) if rd is not None and which != "specular" else (False, 0)
        samples = fd.W * (fd.y1 - fd.y0) * fd.spp if fd is not None else 0
        full = photons_workspace(samples, depth, cap, path, env) if photons else (queues(cap, path, env) if depth else 0)
        return full - 1 if which == "short" else full

    got = {}
    for name, fd, rd, kw in variations(binding):
        a = dict(base, **kw)
        scene = scenes[a["scene"]].h if a["scene"] is not None else None
        f, r = C.byref(fd) if fd is not None else None, C.byref(rd) if rd is not None else None
        out = C.c_uint64(0)
        for entry in ENTRIES:
            nbytes = a["bytes"] if isinstance(a["bytes"], int) else need("photons" in entry, fd, rd, a["bytes"])
            if entry == "mr_render_recursion_workspace":
                st = L.mr_render_recursion_workspace(r, C.byref(out))
            elif entry == "mr_render_recursion":
                st = L.mr_render_recursion(scene, f, r, a["rgb"], a["ws"], nbytes, a["counts"], None)
            elif entry == "mr_render_recursion_photons_workspace":
                st = L.mr_render_recursion_photons_workspace(f, r, C.byref(out))
            else:
                st = L.mr_render_recursion_photons(scene, f, r, a["g"], a["c"], a["dist"], a["k"], a["rgb"], a["ws"], nbytes, a["counts"], None)
            got["%s/%s" % (entry, name)] = {"status": int(st), "message": L.mr_last_error().decode() if st != binding.MR_OK else ""}
    fd, rd = frame_desc(binding), rdesc()                                         # and the two queries' own argument
    for entry, args in ((ENTRIES[0], (C.byref(rd), None)), (ENTRIES[2], (C.byref(fd), C.byref(rd), None))):
        st = getattr(L, entry)(*args)
        got["%s/null_bytes" % entry] = {"status": int(st), "message": L.mr_last_error().decode()}
    assert scenes["host"].info().n_triangles == 1 and g.count() == 0              # the refused calls left scene and maps alone
    return got


def test_statuses_and_messages_are_the_recorded_ones(miro):
    from miro_amd import binding
    with open(GOLDEN) as fh:
        want = json.load(fh)
    got = run(miro)
    assert sorted(got) == sorted(want)
    for case in sorted(want):
        assert got[case] == want[case], case
    # the table reaches what it is meant to hold: every status, and a render call that gets as far as the scene's state
    assert {v["status"] for v in want.values()} == {binding.MR_OK, binding.MR_ERR_INVALID, binding.MR_ERR_STATE}
    assert want["mr_render_recursion/children_0_at_depth_0"]["status"] == binding.MR_ERR_STATE
    assert want["mr_render_recursion_photons/good"]["status"] == binding.MR_ERR_STATE


if __name__ == "__main__":                                                        # records the fixture: see the docstring
    for path in (ROOT, os.path.join(ROOT, "cse168-raytracer_amd"), os.path.join(ROOT, "tests")):
        sys.path.insert(0, path)
    import miro_amd
    miro_amd.load_library()
    with open(GOLDEN, "w") as fh:
        json.dump(run(miro_amd), fh, indent=1, sort_keys=True)
        fh.write("\n")
    print("wrote", GOLDEN)
