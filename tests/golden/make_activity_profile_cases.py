"""Builds tests/golden/activity_profile_cases.json from the reference's own test files (run where the reference tree is at
hand: pass its root as the argument).  Only parameters and expected values are recorded, the literals in source order:
  tests/band_pass_activity_profile_unit_tests.rs
    make_kernel_creation           every call: sigma, the maximum filter size, the expected kernel (:254-473)
    make_band_pass_test            the four parameter lists of its grid (:95-99); MAX_PROB_PROPAGATION_DISTANCE (:28)
    make_band_pass_composition     its two parameter lists (:224-225)
  tests/activity_profile_unit_tests.rs
    run_test_soft_clips            its parameter lists (:517-527), the starts as offsets from the contig's end where they are
  tests/resources/large/human_g1k_v37.20.21.fasta.fai   the length of the first contig (what the tests call contig_len)"""
import json
import os
import re
import sys

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "activity_profile_cases.json")
NUM = r"[-+]?\d+\.?\d*(?:[eE][-+]?\d+)?"


def numbers(text, conv=float):
    return [conv(x) for x in re.findall(NUM, text)]


def main():
    root = sys.argv[1]
    text = open(os.path.join(root, "tests", "band_pass_activity_profile_unit_tests.rs")).read()
    out = {"contig_len": int(open(os.path.join(root, "tests", "resources", "large", "human_g1k_v37.20.21.fasta.fai")).readline().split("\t")[1])}
    out["max_prob_propagation_distance"] = int(re.search(r"MAX_PROB_PROPAGATION_DISTANCE: usize = (\d+)", text).group(1))
    body = text[text.index("fn make_kernel_creation"):]
    out["kernel_creation"] = [dict(sigma=float(m.group(1)), max_size=int(m.group(2)), expected=numbers(m.group(3)))
                              for m in re.finditer(r"test_kernel_creation\(\s*(%s),\s*(\d+),\s*contig_len,\s*vec!\[(.*?)\],?\s*\);" % NUM, body, re.S)]
    grid = text[text.index("fn make_band_pass_test"):text.index("fn band_pass_in_one_pass")]
    lists = re.findall(r"for (\w+) in vec!\[(.*?)\]", grid, re.S)
    out["band_pass_test"] = {name: ([x.strip() == "true" for x in vals.split(",")] if "true" in vals else
                                    [17.0 if "DEFAULT_SIGMA" in x else float(x) for x in vals.split(",") if x.strip()] if name == "sigma" else
                                    numbers(vals, int)) for name, vals in lists}
    comp = text[text.index("fn make_band_pass_composition"):text.index("fn test_kernel_creation")]
    lists = re.findall(r"for (\w+) in vec!\[(.*?)\]", comp, re.S)
    out["band_pass_composition"] = {name: [50 if "MAX_FILTER_SIZE" in x else int(x) for x in vals.split(",") if x.strip()] for name, vals in lists}
    text = open(os.path.join(root, "tests", "activity_profile_unit_tests.rs")).read()
    soft = text[text.index("fn run_test_soft_clips"):]
    soft = soft[:soft.index("// ----")]
    lists = re.findall(r"for (\w+) in vec!\[(.*?)\]", soft, re.S)
    out["soft_clips"] = {name: [x.strip().replace(" ", "") for x in vals.split(",") if x.strip()] if name == "start" else numbers(vals, int)
                         for name, vals in lists}
    json.dump(out, open(OUT, "w"), indent=1)
    print(OUT, {k: (len(v) if hasattr(v, "__len__") else v) for k, v in out.items()})


if __name__ == "__main__":
    main()
