"""Register / scratch budget of every kernel of the product build, from hipcc's -Rpass-analysis=kernel-resource-usage remarks
(written next to the objects by the Makefile).  `python tools/kernel_budget.py --write` records the current build as
tests/golden/kernel_budget.json -- to be done only for a tree whose GPU suite (pytest -m gpu, incl. the fuzz cases) is green:
tests/test_build_budget.py then holds every later build to what was verified on hardware."""
import glob
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAT = re.compile(r"Function Name: (\S+).*?TotalSGPRs: (\d+).*?VGPRs: (\d+).*?ScratchSize \[bytes/lane\]: (\d+).*?Dynamic Stack: (\w+).*?"
                 r"Occupancy \[waves/SIMD\]: (\d+).*?SGPRs Spill: (\d+).*?VGPRs Spill: (\d+)", re.S)
MANIFEST = os.path.join(ROOT, "tests", "golden", "kernel_budget.json")


def _records(path, unit):
    return {"%s:%s" % (unit, name): {"vgprs": int(vgprs), "scratch_bytes_per_lane": int(scratch), "dynamic_stack": dyn == "True",
                                     "waves_per_simd": int(occ), "sgprs_spilled": int(sspill), "vgprs_spilled": int(vspill)}
            for name, sgprs, vgprs, scratch, dyn, occ, sspill, vspill in PAT.findall(open(path).read())}


def current(build_dir=None):
    build_dir = build_dir or os.path.join(ROOT, "cse168-raytracer_amd", "build")
    out = {}
    for f in sorted(glob.glob(os.path.join(build_dir, "*.resource-usage.txt"))):
        out.update(_records(f, os.path.basename(f).replace(".resource-usage.txt", "")))
    return out


def unit_kernels(unit, build_dir=None):
    """The kernels of a unit whose remarks the Makefile keeps out of *.resource-usage.txt (REMARK_UNITS): build/<unit>.remarks.txt"""
    path = os.path.join(build_dir or os.path.join(ROOT, "cse168-raytracer_amd", "build"), unit + ".remarks.txt")
    assert os.path.exists(path), "build the library first (__graft_entry__.build())"
    return _records(path, unit)


def assert_inside_envelope(cur, record, also_main=True):
    """Every kernel of `cur`: known to tests/golden/<record>; no dynamic stack; no more spilled VGPRs, no more scratch per lane
    and no fewer waves per SIMD than its own record -- and, with also_main, than the worst value among the kernels of
    tests/golden/kernel_budget.json as well."""
    rec = json.load(open(os.path.join(ROOT, "tests", "golden", record)))["kernels"]
    assert not sorted(set(cur) - set(rec)), "kernels without a verified record"
    worst = dict(vgprs_spilled=float("inf"), scratch=float("inf"), waves=0)
    if also_main:
        old = json.load(open(MANIFEST))["kernels"].values()
        worst = dict(vgprs_spilled=max(v["vgprs_spilled"] for v in old), scratch=max(v["scratch_bytes_per_lane"] for v in old),
                     waves=min(v["waves_per_simd"] for v in old))
    for name, c in cur.items():
        r = rec[name]
        assert not c["dynamic_stack"], name
        assert c["vgprs_spilled"] <= min(r["vgprs_spilled"], worst["vgprs_spilled"]), (name, c, r)
        assert c["scratch_bytes_per_lane"] <= min(r["scratch_bytes_per_lane"], worst["scratch"]), (name, c, r)
        assert c["waves_per_simd"] >= max(r["waves_per_simd"], worst["waves"]), (name, c, r)


def write_unit(unit):
    """`--write-unit UNIT`: records the kernels of a REMARK_UNITS unit as tests/golden/kernel_budget_<UNIT minus "mr_">.json, under
    the same condition as --write"""
    cur = unit_kernels(unit)
    path = os.path.join(ROOT, "tests", "golden", "kernel_budget_%s.json" % unit.replace("mr_", "", 1))
    json.dump({"note": "recorded from a build whose GPU run of the unit's test file was green; regenerate with tools/kernel_budget.py "
                       "--write-unit %s after re-verifying on the GPU" % unit, "kernels": cur}, open(path, "w"), indent=1, sort_keys=True)
    print("wrote %d kernels to %s" % (len(cur), path))


if __name__ == "__main__":
    if "--write-unit" in sys.argv:
        write_unit(sys.argv[sys.argv.index("--write-unit") + 1])
        sys.exit(0)
    cur = current()
    if "--write" in sys.argv:
        json.dump({"note": "recorded from a build whose GPU suite was green; regenerate with tools/kernel_budget.py --write after "
                           "re-verifying on the GPU", "kernels": cur}, open(MANIFEST, "w"), indent=1, sort_keys=True)
        print("wrote %d kernels to %s" % (len(cur), MANIFEST))
    else:
        worst = sorted(cur.items(), key=lambda kv: -kv[1]["vgprs_spilled"])[:10]
        for k, v in worst:
            print(k[:110], v)
