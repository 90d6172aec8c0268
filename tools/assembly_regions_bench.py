"""phmm_assembly_regions behind phmm_activity_profile on activity_bench's workload A (one window of 200 000 positions x 16
samples, 150-base reads at 30x per sample): the profile lists and the staged reads pass straight through.  Two shapes: ONE
profile over the whole window (the serial regions_cut_kernel has a single wave to run), and the same window in profiles of
--profile-size positions.  Ten calls each after warm-up; prints one JSON line: what came out (regions, active ones, forced
ones, memberships, regions over the depth cap) and, on the host clock, the call that asks for the sizes (all capacities 0) and
the call that fills arrays of exactly those sizes (median and min).  The kernels' own times come from ONE run under
`rocprofv3 --kernel-trace --stats --output-format csv -- python tools/assembly_regions_bench.py`, turned into a table by --trace.
usage: python tools/assembly_regions_bench.py [--steps K] [--warmup W] [--positions N] [--samples S] [--profile-size P]
       python tools/assembly_regions_bench.py --trace <rocprof dir> [--trace-out FILE]   the table of that run's regions_*_kernel times"""
import argparse
import csv
import glob
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import activity_bench  # noqa: E402
from lorikeet_amd import HipPairHMMEngine, PhmmError, activity  # noqa: E402
from lorikeet_amd.genotype import pseudo_counts  # noqa: E402

regions = importlib.import_module("lorikeet_amd.assembly_regions")


def trace_table(directory, out):
    """per kernel of a rocprofv3 kernel trace (CSV) and launch shape: launches, median and minimum of the last ten, in ns"""
    rows = {}
    for path in glob.glob(os.path.join(directory, "**", "*kernel_trace.csv"), recursive=True):
        for r in csv.DictReader(open(path)):
            if "regions_" in r["Kernel_Name"]:
                shape = "x".join(str(r.get(c, "?")) for c in ("Grid_Size_X", "Workgroup_Size_X"))
                name = r["Kernel_Name"].replace("phmm::(anonymous namespace)::", "").replace("(phmm::RegionsParams)", "")
                rows.setdefault("%s [%s]" % (name, shape), []).append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]) - int(r["Start_Timestamp"])))
    lines = ["== rocprofv3 --kernel-trace --stats -- python tools/assembly_regions_bench.py : the window as ONE profile, then in profiles of",
             "   --profile-size positions; a kernel whose launch shape differs between the two has a row for each (the grid counts",
             "   work-items: regions_cut_kernel [64x64] is the one profile), the others one row over both ==",
             "%-48s %6s %12s %12s   (the last ten launches; [grid x, block x])" % ("kernel", "calls", "median_ns", "min_ns")]
    for name, d in sorted(rows.items(), key=lambda kv: min(kv[1])[0]):
        last = [x[1] for x in sorted(d)][-10:]
        lines.append("%-48s %6d %12d %12d" % (name[:48], len(d), int(np.median(last)), min(last)))
    text = "\n".join(lines) + "\n"
    if out:
        open(out, "w").write(text)
    print(text, end="")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--positions", type=int, default=200000)
    ap.add_argument("--samples", type=int, default=16)
    ap.add_argument("--profile-size", type=int, default=10000)
    ap.add_argument("--trace")
    ap.add_argument("--trace-out")
    a = ap.parse_args()
    if a.trace:
        return trace_table(a.trace, a.trace_out)
    packed = activity_bench.window(a.positions, a.samples)
    eng = HipPairHMMEngine(0)
    out = {"tool": "assembly_regions_bench", "positions": a.positions, "samples": a.samples, "reads": int(len(packed["read_pos"])),
           "steps": a.steps, "warmup": a.warmup}
    omit = ("read_counts", "ref_depth", "non_ref_depth", "gl", "pl", "soft_clip_mean", "soft_clip_count", "qual", "af_flags", "is_active_prob")
    for name, size in (("one_profile", 0), ("profiles_of_%d" % a.profile_size, a.profile_size)):
        res = activity.activity_profile(eng, packed, ploidy=2, min_base_quality=10, pseudo_counts=pseudo_counts(), stand_min_conf=30.0,
                                        profile_size=size, omit=omit)
        arrays = regions.from_activity(res, packed, profile_size=size)
        ask, fill, got = [], [], None
        for i in range(a.warmup + a.steps):
            t0 = time.perf_counter()
            try:
                regions.assembly_regions(eng, arrays, capacity=(0, 0))
                required = (0, 0)
            except PhmmError as e:
                required = tuple(int(x) for x in e.required)
            t1 = time.perf_counter()
            got = regions.assembly_regions(eng, arrays, capacity=required)
            t2 = time.perf_counter()
            if i >= a.warmup:
                ask.append(t1 - t0)
                fill.append(t2 - t1)
        flags = got["region_flags"]
        out[name] = {"profiles": int(len(arrays["profile_len"])), "states": int(arrays["profile_len"].sum()),
                     "regions": int(got["required"][0]), "memberships": int(got["required"][1]),
                     "active": int((flags & regions.ACTIVE != 0).sum()), "forced": int((flags & regions.FORCED != 0).sum()),
                     "over_depth": int((flags & regions.OVER_DEPTH != 0).sum()), "failed_profiles": int((got["profile_status"] < 0).sum()),
                     "staged_mb": round(sum(np.asarray(arrays[k]).nbytes for k, _ in regions.PROFILE_INPUTS + regions.READ_INPUTS) / 1e6, 1),
                     "ask_ms_median": round(float(np.median(ask)) * 1e3, 3), "ask_ms_min": round(min(ask) * 1e3, 3),
                     "fill_ms_median": round(float(np.median(fill)) * 1e3, 3), "fill_ms_min": round(min(fill) * 1e3, 3)}
    eng.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
