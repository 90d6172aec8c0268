"""Builds tests/golden/assembly_graph_cases.json from the reference's own files (run where the reference tree is at hand: pass
its root as the argument).  Only the literal sequences, k and expected values of its tests are recorded:
  tests/read_threading_graph_unit_tests.rs
    test_simple_haplotype_rethreading                         k, the two sequences, the expected vertex count, the k-mer looked up
    test_non_unique_middle, test_read_creation_non_unique     k, the reference, the reads, the expected non-unique k-mers
    test_counting_of_start_edges                              k, the sequences, the multiplicities inside and outside the header
    test_counting_of_start_edges_with_multiple_prefixes       k, the sequences, the targets with multiplicity 1 and 3 (2 elsewhere)
    test_cycles_in_graph                                      the reference, the alternate, read length, step, quality, the two k
  src/graphs/multi_sample_edge.rs                             the doc comment's example: capacity 1, 1 / 2 / 2 / 3
The sequences and numbers are read from the files; what each test asserts about them is written down here by hand."""
import json
import os
import re
import sys

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "assembly_graph_cases.json")


def body(text, name):
    at = text.index("fn %s(" % name)
    return text[at:text.find("\n}\n", at)]


def strings(b, *names):
    return [re.search(r'let %s = "([^"]*)"' % n, b).group(1) for n in names]


def main(root):
    t = open(os.path.join(root, "tests", "read_threading_graph_unit_tests.rs")).read()
    k = lambda b: int(re.search(r"default_with_kmer_size\((\d+)\)", b).group(1))  # noqa: E731
    listed = lambda b, name: re.findall(r'"([^"]*)"', re.search(r"let %s = vec!\[([^\]]*)\]" % name, b).group(1))  # noqa: E731
    out = {}
    b = body(t, "test_simple_haplotype_rethreading")
    ref, alt = strings(b, "reference", "alternate")
    out["test_simple_haplotype_rethreading"] = dict(k=k(b), reference=ref, sequences=[alt], n_vertices=len(ref) - k(b) + 1 + k(b),
                                                    find_kmer=dict(sequence=0, start=20))
    for name in ("test_non_unique_middle", "test_read_creation_non_unique"):
        b = body(t, name)
        ref, r1, r2 = strings(b, "reference", "read1", "read2")
        out[name] = dict(k=k(b), reference=ref, sequences=[r1, r2], non_unique=re.findall(r'Kmer::new\(b"([^"]*)"\)', b))
    b = body(t, "test_counting_of_start_edges")
    ref, r1 = strings(b, "reference", "read1")
    out["test_counting_of_start_edges"] = dict(k=k(b), reference=ref, sequences=[r1], header_base="N", header_multiplicity=1, other_multiplicity=2)
    b = body(t, "test_counting_of_start_edges_with_multiple_prefixes")
    ref, a1, r1 = strings(b, "reference", "alt1", "read1")
    out["test_counting_of_start_edges_with_multiple_prefixes"] = dict(
        k=k(b), through_branches=True, reference=ref, sequences=[a1, r1], one_count_targets=listed(b, "one_count_vertices"),
        three_count_targets=listed(b, "three_count_vertices"), other_multiplicity=2)
    b = body(t, "test_cycles_in_graph")
    ref, alt = strings(b, "reference", "alternate")
    out["test_cycles_in_graph"] = dict(reference=ref, alternate=alt, read_length=100, step=20, quality=30, k_with_cycle=25, k_without_cycle=75)
    out["multi_sample_edge_doc"] = dict(capacity=1, creation=1, steps=[["inc", 1], ["pruning", 1], ["flush"], ["pruning", 2], ["inc", 3],
                                                                       ["pruning", 2], ["flush"], ["pruning", 3]])
    json.dump(out, open(OUT, "w"), indent=1)


if __name__ == "__main__":
    main(sys.argv[1])
