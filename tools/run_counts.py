"""How often does a wave of the fused frame stay on the scalar side?  Needs the counting build of mr_frame.hip:
    make -C cse168-raytracer_amd VARIANT=_runc FRAME_DEFS=-DMIRO_RUN_COUNTS
    MIRO_LIB=cse168-raytracer_amd/lib_runc/libmiro_hip.so python tools/run_counts.py
Prints, for one frame, the wave-level node visits, those taken inside uniform_run (mr_traverse.h) and the runs that ended on a
split decision, and how the uniform walks go: how many hold every working lane of their wave, the
leaves and pops they take, and how they end (item 23); and the wave-level triangle tests of the uniform leaf loops that carry the
rejection guard, with those the guard skipped (item 24)."""
import argparse
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "cse168-raytracer_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import miro_amd  # noqa: E402
from miro_amd import binding, scenes  # noqa: E402
from miro_amd import frame as mframe  # noqa: E402


# Stats of the counting build (mr_traverse.h), in its order
COUNTERS = ("node_steps", "run_visits", "run_splits", "walks", "walks_whole", "end_leaf", "end_pop", "end_irregular", "end_far_node",
            "end_done", "walk_leaves", "pops_agree", "pops_differ", "tri_uniform", "tri_skipped")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", default="sponza")
    ap.add_argument("--w", type=int, default=1920)
    ap.add_argument("--h", type=int, default=1080)
    ap.add_argument("--spp", type=int, default=64)
    a = ap.parse_args()
    L = binding.lib()
    if not hasattr(L, "mr_debug_run_counts_b256"):
        raise SystemExit("this library was not built with -DMIRO_RUN_COUNTS")
    d = scenes.SCENES[a.scene]
    sc = miro_amd.Scene(0)
    scenes.populate(sc, d)
    sc.build(4)
    fr = mframe.FusedFrame(sc, d, a.w, a.h, spp=a.spp)
    fr.step()
    torch.cuda.synchronize()
    tot = np.zeros(len(COUNTERS), np.uint64)
    for entry in ("mr_debug_run_counts_b256", "mr_debug_run_counts_b128"):
        buf = np.zeros(len(COUNTERS), np.uint64)
        rc = getattr(L, entry)(buf.ctypes.data_as(C.c_void_p))
        assert rc == 0, rc
        tot += buf
    c = dict(zip(COUNTERS, (int(v) for v in tot)))
    steps, run, splits = c["node_steps"], c["run_visits"], c["run_splits"]
    print("%s %dx%dx%d: %d wave-level node visits, %d of them (%.1f %%) inside runs; %d runs (%.2f %% of the run visits) ended on a split decision" % (
        a.scene, a.w, a.h, a.spp, steps + run, run, 100.0 * run / max(steps + run, 1), splits, 100.0 * splits / max(run, 1)))
    # the uniform walk.  A walk is what a run was, carried on through the leaves and pops it may take:
    # each leaf taken and each pop taken with one value popped is a place where the run before ended and the next one began.
    walks = max(c["walks"], 1)
    print("  %d walks, %d of them (%.1f %%) whole; inside walks: %d leaves, %d pops with one value, %d pops with several" % (
        c["walks"], c["walks_whole"], 100.0 * c["walks_whole"] / walks, c["walk_leaves"], c["pops_agree"], c["pops_differ"]))
    print("  walks ended: %d split decision, %d lanes parted at a pop, %d every lane done, %d at a leaf they may not take, "
          "%d at a pop they may not take, %d irregular node, %d node beyond the run's offsets" % (
              splits, c["pops_differ"], c["end_done"], c["end_leaf"], c["end_pop"], c["end_irregular"], c["end_far_node"]))
    taken = c["walk_leaves"] + c["pops_agree"] - c["end_done"]
    print("  run boundaries of the walk-less kernel: %d; carried through by the walk: %d (%.1f %%)" % (
        c["walks"] + taken, taken, 100.0 * taken / max(c["walks"] + taken, 1)))
    # the rejection guard of the uniform leaf loops (item 24): eye rays in the walk's leaf loop and in leaf_step's scalar arm, shadow
    # rays in leaf_step's scalar arm
    waves = a.w * a.h * a.spp / 64.0
    print("  guarded wave-level triangle tests: %d (%.2f per 64 samples), %d of them (%.1f %%) skipped by the guard" % (
        c["tri_uniform"], c["tri_uniform"] / waves, c["tri_skipped"], 100.0 * c["tri_skipped"] / max(c["tri_uniform"], 1)))


if __name__ == "__main__":
    main()
