"""Builds tests/golden/assembly_kmer_cases.json from the reference's own test files (run where the reference tree is at hand:
pass its root as the argument).  Only the literal sequences, k and expected values of its tests are recorded:
  tests/read_threading_graph_unit_tests.rs
    test_non_unique_middle, test_read_creation_non_unique     k, the reference, the reads, the expected non-unique k-mers
    test_counting_of_start_edges, test_counting_of_start_edges_with_multiple_prefixes
                                                              k, the reference, the reads (sequences added whole, no qualities)
    test_Ns_in_reads_are_not_used_for_graph                   k, the length, the reference base, the quality: read i is the
                                                              reference with an N at i, for every i
  tests/read_threading_assembler_unit_tests.rs
    test_ref_creation, test_ref_non_unique_creation, test_starts_in_middle     k, reference, reads (quality 30 from
                                                              TestAssembler::add_sequence), expected: one vertex spelling `linear`
    test_mismatch_in_first_kmer                               k, reference, reads"""
import json
import os
import re
import sys

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "assembly_kmer_cases.json")


def body(text, name):
    at = text.index("fn %s(" % name)
    end = text.find("\n}\n", at)
    return text[at:end]


def main():
    root = sys.argv[1]
    out = {}
    text = open(os.path.join(root, "tests", "read_threading_graph_unit_tests.rs")).read()
    for name in ("test_non_unique_middle", "test_read_creation_non_unique", "test_counting_of_start_edges",
                 "test_counting_of_start_edges_with_multiple_prefixes"):
        b = body(text, name)
        case = dict(k=int(re.search(r"default_with_kmer_size\((\d+)\)", b).group(1)),
                    reference=re.search(r'let reference = "(\w+)"', b).group(1),
                    reads=re.findall(r'let (?:read|alt)\d+ = "(\w+)"', b))
        m = re.search(r"assert_non_uniques\(&mut assembler, vec!\[(.*?)\]", b, re.S)
        if m:
            case["non_unique"] = re.findall(r'Kmer::new\(b"(\w+)"\)', m.group(1))
        out[name] = case
    b = body(text, "test_Ns_in_reads_are_not_used_for_graph")
    out["test_Ns_in_reads_are_not_used_for_graph"] = dict(
        k=int(re.search(r"default_with_kmer_size\((\d+)\)", b).group(1)), length=int(re.search(r"let length = (\d+)", b).group(1)),
        base=re.search(r"vec!\[b'(\w)'; length\]", b).group(1), quality=int(re.search(r"let quals = vec!\[(\d+); length\]", b).group(1)),
        expected_paths=int(re.search(r"assert_eq!\(paths.len\(\), (\d+)\)", b).group(1)))
    text = open(os.path.join(root, "tests", "read_threading_assembler_unit_tests.rs")).read()
    quality = int(re.search(r"let quals = vec!\[(\d+); bases.len\(\)\]", body(text, "add_sequence")).group(1))
    for name in ("test_ref_creation", "test_ref_non_unique_creation", "test_starts_in_middle", "test_mismatch_in_first_kmer"):
        b = body(text, name)
        case = dict(k=int(re.search(r"TestAssembler::new\((\d+)\)", b).group(1)), reference=re.search(r'let reference = "(\w+)"', b).group(1),
                    reads=re.findall(r'let alternate\d* = "(\w+)"', b), quality=quality)
        if "assert_linear_graph(&mut assembler, reference.to_string())" in b:
            case["linear"] = case["reference"]
        out[name] = case
    json.dump(out, open(OUT, "w"), indent=1, sort_keys=True)
    open(OUT, "a").write("\n")
    print("%d cases -> %s" % (len(out), OUT))


if __name__ == "__main__":
    main()
