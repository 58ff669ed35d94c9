"""Wall time of mr_bvh_build from call to return, upload included, host builder (builder 0) against device builder (builder 1,
csrc/mr_bvh_build.hip), leaf size 4, in one process: builder 1 once for warm-up, then the two alternate and the median of
--reps runs of each is taken (--host-reps for the host builder on scenes above --large objects, whose host build takes many
seconds).  The phases are those of mr_bvh_build_timing.  The two trees are compared (export_tree, bit for bit) before anything is
timed.  Every build runs under a time limit of its own (the process is ended if one exceeds --step-seconds).  One JSON line per
scene, printed and appended to --out.
usage: python tools/bvh_build_probe.py [--scenes teapot,bunny,sponza,bunny20] [--reps 5] [--out profiles/bvh_build_line.json]"""
import argparse, json, os, signal, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "cse168-raytracer_amd"))
import numpy as np, torch
import miro_amd
from miro_amd import scenes

ap = argparse.ArgumentParser()
ap.add_argument("--scenes", default="teapot,bunny,sponza,bunny20")
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--host-reps", type=int, default=1)
ap.add_argument("--large", type=int, default=500000)
ap.add_argument("--step-seconds", type=float, default=120.0)
ap.add_argument("--out", default="")
a = ap.parse_args()

signal.signal(signal.SIGALRM, signal.SIG_DFL)                      # the default action ends the process, also inside the runtime


def build(sc, builder):
    """one mr_bvh_build; a build that takes longer than --step-seconds ends the process"""
    signal.setitimer(signal.ITIMER_REAL, a.step_seconds)
    try:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        sc.build(4, builder=builder)
        torch.cuda.synchronize()
        r = sc.build_timing()
        r["wall_ms"] = (time.perf_counter() - t0) * 1e3
        assert r.pop("builder") == builder
        return r
    finally:
        signal.setitimer(signal.ITIMER_REAL, 0)


def median_of(runs):
    return {k: round(float(np.median([r[k] for r in runs])), 3) for k in runs[0]}


assert torch.cuda.is_available(), "the probe measures on the GPU"
for name in a.scenes.split(","):
    sc = miro_amd.Scene(0)
    scenes.populate(sc, name)
    build(sc, 1)                                                    # warm-up: code objects, allocator
    dev_tree, dev_info = sc.export_tree(), sc.info()
    first_host = build(sc, 0)
    host_tree, info = sc.export_tree(), sc.info()
    assert (info.n_nodes, info.n_leaves, info.max_depth) == (dev_info.n_nodes, dev_info.n_leaves, dev_info.max_depth)
    assert all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(dev_tree, host_tree)), "the trees differ"
    host_reps = a.reps if info.n_triangles <= a.large else a.host_reps
    host, dev = [first_host] if info.n_triangles > a.large else [], []
    for rep in range(a.reps):
        dev.append(build(sc, 1))
        if len(host) < host_reps:
            host.append(build(sc, 0))
    h, d = median_of(host), median_of(dev)
    line = dict(tool="bvh_build_probe", scene=scenes.sponza_label() if name == "sponza" else name, leaf_size=4, device=torch.cuda.get_device_name(0),
                objects=info.n_triangles, nodes=info.n_nodes, max_depth=info.max_depth, host=h, device_builder=d, host_runs=len(host),
                device_runs=len(dev), speedup=round(h["wall_ms"] / d["wall_ms"], 2),
                host_wall_ms_runs=[round(x["wall_ms"], 2) for x in host], device_wall_ms_runs=[round(x["wall_ms"], 2) for x in dev])
    print(json.dumps(line), flush=True)
    if a.out:
        with open(a.out, "a") as fh:
            fh.write(json.dumps(line) + "\n")
    sc.close()
