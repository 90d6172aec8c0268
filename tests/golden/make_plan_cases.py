"""Builds tests/golden/plan_cases.json: the launch plan (every field of phmm_plan_info but `reserved`) the planner makes of a
fixed set of seeded synthetic batches, through phmm_plan_describe -- host only, no GPU, milliseconds per case.

Run it against a library built from the commit whose plans are to be pinned (the fixture in the tree was recorded before the
planner moved out of phmm_api.cpp); tests/test_plan_cases.py then holds every later planner to it.  The batches are described,
not stored: [kind, arguments ...] of lorikeet_amd/synthetic.py, which tests/test_plan_cases.py::build_batch makes again."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))                     # tests/
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))    # the repository

SMALL = [3, 24, None, 90, [40, 50, 60], 1]   # make_regions(3, 24, nh, 90, [40, 50, 60], seed=1)


def case(name, batch, env=None, f32_first=False, concurrent_callers=1):
    return {"name": name, "batch": batch, "env": {k: str(v) for k, v in (env or {}).items()}, "f32_first": f32_first,
            "concurrent_callers": concurrent_callers}


def cases():
    out = [case("config2(%d)" % n, ["config2", n]) for n in (1, 2, 8, 32, 128, 1024)]
    out += [case("ragged", ["ragged"]), case("ragged f32-first", ["ragged"], f32_first=True),
            case("ragged callers=8", ["ragged"], concurrent_callers=8), case("config5", ["config", "config5"])]
    for nh in (5, 7, 9):   # haplotype counts that leave the last wave of a 16-lane class partly empty
        b = ["make_regions"] + [nh if x is None else x for x in SMALL]
        out += [case("3x24x%d chain=4" % nh, b, {"PHMM_FORCE_CHAIN": 4}),
                case("3x24x%d chain=4 L=16" % nh, b, {"PHMM_FORCE_CHAIN": 4, "PHMM_FORCE_L": 16}),
                case("3x24x%d chain=4 L=16 streams=2" % nh, b, {"PHMM_FORCE_CHAIN": 4, "PHMM_FORCE_L": 16, "PHMM_FORCE_STREAMS": 2}),
                case("3x24x%d chain=4 L=16 f32-first" % nh, b, {"PHMM_FORCE_CHAIN": 4, "PHMM_FORCE_L": 16}, f32_first=True)]
    h300 = ["make_regions", 3, 24, 3, 300, [40, 50, 60], 1]
    out += [case("3x24x3 H=300 L=32", h300, {"PHMM_FORCE_L": 32}),
            case("3x24x3 H=300 L=32 chain=8", h300, {"PHMM_FORCE_L": 32, "PHMM_FORCE_CHAIN": 8})]
    out += [case("generic: read of 2400", ["make_regions", 1, 2, 2, 50, [2400], 1]),     # too long for the LDS rows
            case("generic: haplotype of 2100", ["make_regions", 1, 2, 2, 2100, [50], 1]),  # no instantiated K
            case("empty regions", ["empty_regions"]),                                      # no reads / no haplotypes, between two ordinary ones
            case("smoke", ["make_regions", 2, 16, 3, 90, [40, 50, 60], 11])]
    return out


def main():
    path = os.path.join(HERE, "plan_cases.json")
    if not os.path.exists(path):   # (the test module reads the fixture when it is imported)
        with open(path, "w") as f:
            json.dump({"cases": []}, f)
    import test_plan_cases as t
    done = []
    for c in cases():
        c["expect"] = t.describe(c)
        done.append(c)
        print("%-28s %s" % (c["name"], c["expect"]))
    with open(path, "w") as f:
        json.dump({"cases": done}, f, indent=1)
        f.write("\n")
    print("%d cases" % len(done))


if __name__ == "__main__":
    main()
