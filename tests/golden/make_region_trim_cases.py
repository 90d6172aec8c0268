"""Builds tests/golden/region_trim_cases.json from the reference's own test files (run where the reference tree is at hand:
pass its root as the argument).  Only the literal values of its tests are recorded:
  tests/haplotype_unit_tests.rs
    test_trimming          the location, the bases, hap_start of the all-M haplotype trimmed to every sub-span; the haplotype
                           ACT / 1M2D2M and the three spans that give None
    test_trimming_data_with_leading_and_trailing_insertions   the offset and the rows (bases, cigar, start, stop, expected cigar,
                           expected bases)
    test_bad_trim_loc      the location, the bases, the span that is an Err
  tests/alignment_utils_unit_tests.rs
    make_trim_cigar_data   the value lists of its two loop nests and its literal rows (cigar, start, end, expected)
  tests/assembly_result_set_unit_tests.rs
    trimming_data          the active span, the padding, how many haplotypes (one substitution each, at position i); its bases
                           are random there and are not recorded"""
import json
import os
import re
import sys

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "region_trim_cases.json")


def body(text, name):
    at = text.index("fn %s(" % name)
    end = text.find("\n}\n", at)
    return text[at:end]


def ints(s):
    return [int(x) for x in re.findall(r"\d+", s)]


def main():
    root = sys.argv[1]
    out = {}
    text = open(os.path.join(root, "tests", "haplotype_unit_tests.rs")).read()
    b = body(text, "test_trimming")
    out["test_trimming"] = dict(
        loc=ints(re.search(r"let loc = SimpleInterval::new\(0, (\d+, \d+)\)", b).group(1)),
        bases=re.search(r'let full_bases = "(\w+)"', b).group(1), hap_start=int(re.search(r"let hap_start = (\d+)", b).group(1)))
    m = re.search(r'Haplotype::new\("(\w+)"\.as_bytes\(\), false\);\s*full\.set_genome_location\(SimpleInterval::new\(0, (\d+), (\d+)\)\);\s*'
                  r'full\.set_alignment_start_hap_wrt_ref\((\d+)\);\s*full\.set_cigar\(CigarString::try_from\("(\w+)"\)', b)
    out["test_trimming_none"] = dict(
        bases=m.group(1), loc=[int(m.group(2)), int(m.group(3))], hap_start=int(m.group(4)), cigar=m.group(5),
        spans=[ints(s) for s in re.findall(r"test_trim\(full(?:\.clone\(\))?, SimpleInterval::new\(0, (\d+, \d+)\), None\)", b)])
    rows = re.findall(r'test_trim_leading_and_trailing_insertions\("(\w+)", "(\w+)", (\d+), (\d+), "(\w+)", "(\w+)"\)',
                      body(text, "test_trimming_data_with_leading_and_trailing_insertions"))
    out["test_trimming_data_with_leading_and_trailing_insertions"] = dict(
        offset=int(re.search(r"let offset = (\d+)", body(text, "test_trim_leading_and_trailing_insertions")).group(1)),
        rows=[[r[0], r[1], int(r[2]), int(r[3]), r[4], r[5]] for r in rows])
    b = body(text, "test_bad_trim_loc")
    out["test_bad_trim_loc"] = dict(loc=ints(re.search(r"let loc = SimpleInterval::new\(0, (\d+, \d+)\)", b).group(1)),
                                    bases=re.search(r'Haplotype::new\("(\w+)"', b).group(1),
                                    span=ints(re.search(r"hap\.trim\(SimpleInterval::new\(0, (\d+, \d+)\)\)", b).group(1)))
    text = open(os.path.join(root, "tests", "alignment_utils_unit_tests.rs")).read()
    b = body(text, "make_trim_cigar_data")
    ops, pad_ops = [re.findall(r'"(.)"', v) for v in re.findall(r"for (?:op|pad_op) in vec!\[(.*?)\]", b)]
    pads = [ints(v) for v in re.findall(r"for (?:left_pad|right_pad) in vec!\[(.*?)\]", b)]
    out["make_trim_cigar_data"] = dict(
        ops=ops, pad_ops=pad_ops, my_length=ints(re.search(r"for my_length in (\d+\.\.\d+)", b).group(1)),
        pad=ints(re.search(r"for left_pad in (\d+\.\.\d+)", b).group(1)), insertion_pads=pads[0], insertion_right_pads=pads[1],
        insertion_sizes=ints(re.search(r"for ins_size in vec!\[(.*?)\]", b).group(1)),
        rows=[[r[0], int(r[1]), int(r[2]), r[3]] for r in re.findall(r'^\s+test_trim_cigar\("(\w+)", (\d+), (\d+), "(\w+)"\);', b, re.M)])
    text = open(os.path.join(root, "tests", "assembly_result_set_unit_tests.rs")).read()
    b = body(text, "trimming_data")
    m = re.search(r"AssemblyRegion::new\(SimpleInterval::new\(0, (\d+), (\d+)\), true, (\d+), (\d+)", b)
    out["trimming_data"] = dict(active=[int(m.group(1)), int(m.group(2))], padding=int(m.group(3)), contig_length=int(m.group(4)),
                                haplotypes=ints(re.search(r"for test_hap in (\d+\.\.=\d+)", b).group(1)))
    json.dump(out, open(OUT, "w"), indent=1, sort_keys=True)
    open(OUT, "a").write("\n")
    print("%d cases -> %s" % (len(out), OUT))


if __name__ == "__main__":
    main()
