"""Builds tests/golden/read_clipper_cases.json from the reference's own test files (run where the reference tree is at hand:
pass its root as the argument).  Strings and numbers only:
  src/test_utils/read_clipper_test_utils.rs   BASES, QUALS (:11-12); the clip and core element lists (:13-25) from which
                                              generate_cigar_list(6, false) (:87-165) enumerates its CIGARs -- the enumeration is
                                              redone here, in its order, through the restated CigarBuilder; duplicates stay
  src/utils/artificial_read_utils.rs          the artificial read's position (:34)
  tests/read_clipper_unit_tests.rs            the additional CIGAR (:29), the element limit (:28), the grid of
                                              make_revert_soft_clips_before_contig (:340-341) with the CIGARs its format strings
                                              give (:350, :359), the entirely soft-clipped read (:297)
  tests/assembly_based_caller_utils_unit_tests.rs   the two SAM records of test_finalize_region (:55-56), its region (:44) with
                                              the padding (:46) and min_bq (:64)"""
import json
import os
import re
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import finalize_restatement as FR  # noqa: E402

OUT = os.path.join(HERE, "read_clipper_cases.json")
NAMES = {"Ins": "I", "Del": "D", "Match": "M", "RefSkip": "N", "SoftClip": "S", "HardClip": "H"}


def elements(text):
    return [(FR.OPS.index(NAMES[m.group(1)]), int(m.group(2))) for m in re.finditer(r"Cigar::(\w+)\((\d+)\)", text)]


def generate_cigar_list(maximum, leading_clips, core_elements):
    trailing_clips = leading_clips[::-1]
    out = []
    for lead in leading_clips:
        for trail in trailing_clips:
            max_core = maximum - len(lead) - len(trail)
            if max_core < 1:
                continue
            comb, current = [0] * max_core, 0
            while True:
                core = [core_elements[n] for n in comb]
                indel = [op in (FR.I, FR.D) for op, _ in core]
                good = not any(a and b for a, b in zip(indel, indel[1:])) and core[0][0] != FR.D and core[-1][0] != FR.D
                if good:
                    b = FR.CigarBuilder(True)
                    for part in (lead, core, trail):   # add_all: the first Err ends the list
                        for op, n in part:
                            if not b.add(op, n):
                                break
                    made = b.make()
                    if made is not None:
                        out.append(FR.cigar_string(made))
                changed = False
                while current < max_core and comb[current] == len(core_elements) - 1:
                    current += 1
                    changed = True
                if current == max_core:
                    break
                comb[current] += 1
                if changed:
                    for i in range(current):
                        comb[i] = 0
                    current = 0
    return out


def main():
    root = sys.argv[1]
    utils = open(os.path.join(root, "src", "test_utils", "read_clipper_test_utils.rs")).read()
    tests = open(os.path.join(root, "tests", "read_clipper_unit_tests.rs")).read()
    region = open(os.path.join(root, "tests", "assembly_based_caller_utils_unit_tests.rs")).read()
    art = open(os.path.join(root, "src", "utils", "artificial_read_utils.rs")).read()
    out = {}
    out["bases"] = "".join(re.findall(r"'(\w)' as u8", re.search(r"BASES: Vec<u8> = vec!\[(.*?)\];", utils).group(1)))
    out["quals"] = [int(x) for x in re.search(r"QUALS: Vec<u8> = vec!\[(.*?)\];", utils).group(1).split(",")]
    out["position"] = int(re.search(r"fn create_artificial_read\(.*?set_pos\((\d+)\)", art, re.S).group(1))
    lead = re.search(r"LEADING_CLIPS: Vec<Vec<Cigar>> = vec!\[(.*?)\];", utils, re.S).group(1)
    leading_clips = [elements(x) for x in re.findall(r"Vec::new\(\)|vec!\[.*?\]", lead, re.S)]
    core = elements(re.search(r"CORE_CIGAR_ELEMENTS: Vec<Cigar> =\s*vec!\[(.*?)\];", utils, re.S).group(1))
    maximum, skips = re.search(r"generate_cigar_list\((\d+), (\w+)\)", tests).groups()
    assert skips == "false"
    out["maximum_cigar_elements"] = int(maximum)
    out["cigars"] = generate_cigar_list(int(maximum), leading_clips, core) + [re.search(r'try_from\("(\w+)"\)', tests).group(1)]
    out["entirely_soft_clipped"] = re.search(r'fn test_revert_entirely_soft_clipped_reads.*?make_read_from_str\("(\w+)"', tests, re.S).group(1)
    grid = tests[tests.index("fn make_revert_soft_clips_before_contig"):]
    soft_starts, alignment_starts = [[int(x) for x in v.split(",")] for v in re.findall(r"in vec!\[(.*?)\]", grid)[:2]]
    n_matches = int(re.search(r"let n_matches = (\d+);", grid).group(1))
    out["before_contig"] = [dict(soft_start=s, alignment_start=a, cigar="%dS%dM" % (a - s, n_matches),
                                 expected_cigar="%dH%dM" % (1 - s, a + n_matches - 1), expected_start=0)
                            for s in soft_starts for a in alignment_starts]
    body = region[region.index("fn test_finalize_region"):region.index("fn test_get_variant_contexts_from_given_alleles")]
    out["finalize_region"] = dict(
        sam=[m.replace("\\t", "\t") for m in re.findall(r'from_sam\(.*?"((?:[^"\\]|\\.)*)"\.as_bytes', body, re.S)],
        span=[int(x) for x in re.search(r"SimpleInterval::new\(0, (\d+), (\d+)\),\s*true", body).groups()],
        extension=int(re.search(r"true,\s*(\d+),", body).group(1)), min_bq=int(re.search(r"let min_bq = (\d+);", body).group(1)),
        contig_length=int(re.search(r"SimpleInterval::new\(0, 1, (\d+)\)", body).group(1)))
    json.dump(out, open(OUT, "w"), indent=1)
    print(OUT, {k: (len(v) if hasattr(v, "__len__") else v) for k, v in out.items()})


if __name__ == "__main__":
    main()
