"""How often does a wave of the fused frame stay on the scalar side?  Needs the counting build of mr_frame.hip:
    make -C cse168-raytracer_amd VARIANT=_runc FRAME_DEFS=-DMIRO_RUN_COUNTS
    MIRO_LIB=cse168-raytracer_amd/lib_runc/libmiro_hip.so python tools/run_counts.py
Prints, for one frame, the wave-level node visits, those taken inside uniform_run (mr_traverse.h) and the runs that ended on a
split decision."""
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
    tot = np.zeros(3, np.uint64)
    for entry in ("mr_debug_run_counts_b256", "mr_debug_run_counts_b128"):
        buf = np.zeros(3, np.uint64)
        rc = getattr(L, entry)(buf.ctypes.data_as(C.c_void_p))
        assert rc == 0, rc
        tot += buf
    steps, run, splits = (int(v) for v in tot)
    print("%s %dx%dx%d: %d wave-level node visits, %d of them (%.1f %%) inside runs; %d runs (%.2f %% of the run visits) ended on a split decision" % (
        a.scene, a.w, a.h, a.spp, steps + run, run, 100.0 * run / max(steps + run, 1), splits, 100.0 * splits / max(run, 1)))


if __name__ == "__main__":
    main()
