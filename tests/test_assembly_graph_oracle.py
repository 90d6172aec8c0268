"""The serial restatement of the reference's read-threading graph (tests/assembly_graph_restatement.py) held to the reference's
own test literals (tests/golden/assembly_graph_cases.json) and to expectations derived by hand from the cited lines, one per
quirk; a census of what the GPU case sets (tests/assembly_graph_cases.py) reach; and the binding of phmm_assembly_graph in the
library, the header, the ctypes table and the Rust declarations.  CPU only.
Line numbers: R = src/read_threading/read_threading_graph.rs, E = src/graphs/multi_sample_edge.rs of the reference."""
import os
import re
from collections import OrderedDict

import pytest

import assembly_graph_cases as G
import assembly_graph_restatement as R
from lorikeet_amd import _lib
from lorikeet_amd.assembly import assembly_graph  # noqa: F401  (the binding this file is about: without it nothing here runs)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = G.golden()
NONE = R.NO_VERTEX


def test_the_export_is_in_the_library_the_binding_and_the_rust_declarations():
    lib = _lib.load()
    ffi = open(os.path.join(ROOT, "integration", "hip_ffi.rs")).read()
    header = open(os.path.join(ROOT, "include", "phmm.h")).read()
    n = "phmm_assembly_graph"
    assert getattr(lib, n) is not None
    args = next(a for name, _, a in _lib.SYMBOLS if name == n)
    decl = re.search(r"pub fn %s\s*\(([^)]*)\)" % n, ffi, re.S).group(1)
    c_decl = re.search(r"\bint %s\(([^)]*)\)" % n, header, re.S).group(1)
    assert len(args) == len([x for x in decl.split(",") if x.strip()]) == len(c_decl.split(",")) == 35
    for name in ("MAX_SAMPLES", "MAX_PRUNING_SAMPLES", "VERTEX_TRACKED", "VERTEX_REF_SOURCE"):
        value = int(re.search(r"#define PHMM_GRAPH_%s (\d+)u?\b" % name, header).group(1))
        assert getattr(_lib, "PHMM_GRAPH_" + name) == value, name
        assert re.search(r"pub const PHMM_GRAPH_%s: \w+ = %d;" % (name, value), ffi), name
    assert _lib.PHMM_GRAPH_MAX_SAMPLES >= 16 and _lib.PHMM_GRAPH_MAX_PRUNING_SAMPLES >= 4
    assert (G.MAX_SAMPLES, G.MAX_PRUNING_SAMPLES) == (_lib.PHMM_GRAPH_MAX_SAMPLES, _lib.PHMM_GRAPH_MAX_PRUNING_SAMPLES)
    assert (R.TRACKED, R.REF_SOURCE) == (_lib.PHMM_GRAPH_VERTEX_TRACKED, _lib.PHMM_GRAPH_VERTEX_REF_SOURCE)
    backend = open(os.path.join(ROOT, "integration", "hip_backend.rs")).read()
    assert "pub fn assembly_graph(" in backend and "phmm_assembly_graph(" in backend
    import tools.source_hash as SH
    assert {"phmm_graph_internal.hpp", "phmm_graph_kernels.hip"} <= set(SH.KERNEL_SOURCES["graph"])
    assert "graph=%s" % SH.source_hash("graph") in lib.phmm_build_info().decode()
    import lorikeet_amd
    assert lorikeet_amd.assembly_graph is lorikeet_amd.assembly.assembly_graph


# ---- the reference's own literals: sequences added as its tests add them, all under sample 0 ---------------------------------------
def _literal(c, k=None):
    g = R.ReadThreadingGraph(k or c["k"])
    g.set_increase_counts_through_branches(c.get("through_branches", False))
    pending = OrderedDict()
    ref = c["reference"].encode()
    g.add_sequence(pending, "anonymous", 0, ref, 0, len(ref), 1, True)
    for i, s in enumerate(c["sequences"]):
        g.add_sequence(pending, "anonymous", 0, s.encode(), 0, len(s), 1, False, i)
    g.build_graph_if_necessary(pending)
    return g


def test_counting_of_start_edges():
    c = GOLDEN["test_counting_of_start_edges"]
    g = _literal(c)
    header = ord(c["header_base"])
    assert g.weight
    for e, w in enumerate(g.weight):
        in_header = g.vertices[g.edge_source[e]][-1] == header or g.vertices[g.edge_target[e]][-1] == header
        assert w.multiplicity == (c["header_multiplicity"] if in_header else c["other_multiplicity"]), e


def test_counting_of_start_edges_with_multiple_prefixes():
    c = GOLDEN["test_counting_of_start_edges_with_multiple_prefixes"]
    g = _literal(c)
    assert g.increase_counts_through_branches and g.weight
    for e, w in enumerate(g.weight):
        target = g.vertices[g.edge_target[e]].decode()
        want = 1 if target in c["one_count_targets"] else 3 if target in c["three_count_targets"] else c["other_multiplicity"]
        assert w.multiplicity == want, (e, target)
    # the default mode stops at the branch: the walk from TCA finds two in-edges (GTC -> TCA, CTC -> TCA) and adds nothing
    d = _literal(dict(c, through_branches=False))
    assert [w.multiplicity for w in d.weight] != [w.multiplicity for w in g.weight]


def test_simple_haplotype_rethreading():
    c = GOLDEN["test_simple_haplotype_rethreading"]
    g = _literal(c)
    assert len(g.vertices) == c["n_vertices"] != len(c["reference"]) - c["k"] + 1
    f = c["find_kmer"]
    assert R.kmer(c["sequences"][f["sequence"]].encode(), f["start"], c["k"]) in g.kmer_to_vertex_map


@pytest.mark.parametrize("name", ["test_non_unique_middle", "test_read_creation_non_unique"])
def test_the_non_unique_sets_of_the_references_tests(name):
    c = GOLDEN[name]
    assert _literal(c).non_unique_kmers == {s.encode() for s in c["non_unique"]}


def test_cycles_in_graph():
    reg, c = G.cycle_region()
    _, small = R.create_graph(reg["ref"], reg["reads"], c["k_with_cycle"])
    _, large = R.create_graph(reg["ref"], reg["reads"], c["k_without_cycle"])
    assert small.has_cycles() and not large.has_cycles()


def test_the_doc_example_of_multi_sample_edge():
    c = GOLDEN["multi_sample_edge_doc"]
    e = R.MultiSampleEdge(False, c["creation"], c["capacity"])
    for step in c["steps"]:
        if step[0] == "inc":
            e.inc_multiplicity(step[1])
        elif step[0] == "flush":
            e.flush_single_sample_multiplicity()
        else:
            assert e.get_pruning_multiplicity() == step[1], step
    assert e.multiplicity == 5


# ---- one hand-derived expectation per quirk ----------------------------------------------------------------------------------------
def _graph(reg, k, nps=1):
    return R.graph(reg["ref"], reg["reads"], k, 10, reg.get("samples"), nps)


def _weights(x):
    return {(s, t): (m, p) for s, t, _, m, p in x["edges"]}


def test_the_backward_walk_indexes_the_whole_sequence():
    # CTGTCAAG, k = 3: vertices CTG TGT GTC TCA CAA AAG = 0 .. 5.  The read CAGTCAAG has a low-quality base at 1: its run is
    # [2, 8), find_start gives 2 (GTC), which has the one in-edge TGT -> GTC.  R:666 reads original_kmer[offset] with offset
    # k - 2 = 1 of the WHOLE read (R:504): 'A', not the 'T' in front of the start.  TGT's suffix is 'T': no step, the edges in
    # front of GTC keep 1.  The same read cut to its run has 'T' at 1 and 'G' at 0: both steps (TGT's T, CTG's G).
    whole, cut = _graph(G.walk_offset_counts_from_the_sequence_start(), 3), _graph(G.the_same_read_cut_to_its_run(), 3)
    assert [m for _, _, _, m, _ in whole["edges"]] == [1, 1, 2, 2, 2]
    assert [m for _, _, _, m, _ in cut["edges"]] == [2, 2, 2, 2, 2]
    assert whole["read_vertex"] == [[NONE, NONE, 2, 3, 4, 5, NONE, NONE]] and cut["read_vertex"] == [[2, 3, 4, 5, NONE, NONE]]


def test_the_source_kmer_gets_a_fresh_vertex_at_a_later_occurrence_and_the_map_vertex_at_a_start():
    # GATTCCAGT: GAT ATT TTC TCC CCA CAG AGT = 0 .. 6; TTC is non-unique (twice in the read), so vertex 2 is not tracked.  The
    # read TTCCGATTC starts at 1 (TCC = 3), creates CCG = 7 and CGA = 8; GAT is the reference source: get_kmer_vertex(.., false)
    # is None (R:614-615), a fresh vertex 9 that track_kmer finds in the map already (R:636).  ATT merges into 1; from there the
    # edge 1 -> 2 has the suffix C: followed, 2.
    x = _graph(G.source_kmer_again_in_a_read(), 3)
    assert len(x["vertices"]) == 10 and x["vertices"][9] == (1, 4, 0) and x["vertices"][0] == (0, 0, R.TRACKED | R.REF_SOURCE)
    assert x["vertices"][2] == (0, 2, 0)
    assert x["read_vertex"] == [[NONE, 3, 7, 8, 9, 1, 2, NONE, NONE]]
    assert _weights(x)[(9, 1)] == (1, 1) and _weights(x)[(1, 2)] == (2, 1) and (8, 0) not in _weights(x)
    # a read that STARTS on GAT gets the source's own vertex (get_or_create_kmer_vertex allows it, R:600)
    y = _graph(G.source_kmer_starts_a_read(), 3)
    assert len(y["vertices"]) == 7 and y["read_vertex"] == [[0, 1, 2, 3, NONE, NONE]]
    assert [m for _, _, _, m, _ in y["edges"]] == [2, 2, 2, 1, 1, 1]


def test_a_reference_of_exactly_k_bases_threads_nothing():
    # R:492: 4 <= 0 + 4, return -- no vertex, no reference_path, no ref_source.  ACGTTACGTC: ACGT is non-unique, the start is
    # CGTT at 1; the second ACGT gets an untracked vertex.
    x = _graph(G.reference_of_exactly_k(), 4)
    assert x["ref_path"] == [] and x["ref_vertex"] == [NONE] * 4 and x["flags"] == 0
    assert [v[:2] for v in x["vertices"]] == [(1, p) for p in range(1, 7)] and [v[2] for v in x["vertices"]] == [1, 1, 1, 1, 0, 1]
    assert not any(e[2] for e in x["edges"]) and len(x["edges"]) == 5
    assert R.graph(b"ACG", [(b"ACGTACGT", bytes([30] * 8))], 4)["flags"] == R.REF_SHORT


def test_pruning_multiplicities():
    # one sample, capacity 2: the heap holds the creation's 1 and the flushed count, two values, nothing leaves; the peek is 1
    ref = G.region("GATTCCAGTA", ["GATTCCAGTA", "GATTCCAGTA"])
    assert {p for *_, p in _graph(ref, 3, 2)["edges"]} == {1}
    # capacity 1: the larger of the two groups' counts -- the reference's 1 and the sample's 2
    assert {p for *_, p in _graph(ref, 3, 1)["edges"]} == {2}
    # an edge the SECOND group creates is not flushed behind the first (R:454-456 flushes the edges that exist): capacity 3
    # holds {1, 2}, peek 1.  Flushed by the first group too it would hold {1, 0, 2} and answer 0.
    reg = G.region("GATTCCAGTA", ["GATTCCAGTA", "GATTGCAGTA", "GATTGCAGTA"], samples=[5, 2, 2])
    w3, w1 = _weights(_graph(reg, 3, 3)), _weights(_graph(reg, 3, 1))
    assert w3[(1, 8)] == (2, 1) and w1[(1, 8)] == (2, 2)
    # a reference edge all three reads follow: the reference's 1, sample 5's 1, sample 2's 2.  Capacity 3 of {1, 1, 1, 2}: 1
    assert w3[(0, 1)] == (4, 1) and w1[(0, 1)] == (4, 2)


def test_the_group_order_differs_between_two_k():
    # sample 9's first read has 5 bases: a sequence at k = 3, none at k = 6, where its second read comes behind sample 4's first
    reg = G.group_order_differs_between_k()
    assert _graph(reg, 3)["group_order"] == [9, 4] and _graph(reg, 6)["group_order"] == [4, 9]


# ---- what the GPU sets reach ---------------------------------------------------------------------------------------------------
def test_the_gpu_case_sets_reach_every_branch():
    n = G.census(G.calls().values())
    assert all(v > 0 for v in n.values()), n


def test_the_layout_of_the_expected_arrays_with_and_without_windows():
    reg = G.region("CTGTCAAG", [G.read("TTGTCAAGTT")])
    cut = G.region("CTGTCAAG", [G.read("GTCAAG")])
    a, b = G.expected(G.call([reg], [3]), windows=[[(2, 6)]]), G.expected(G.call([cut], [3]))
    assert a["read_vertex"][0].tolist() == [NONE, NONE] + b["read_vertex"][0].tolist() + [NONE, NONE]
    for name in G.SIZES + G.OFFSETS + G.VERTEX + G.EDGE + ("ref_path", "ref_vertex"):
        assert a[name].tolist() == b[name].tolist(), name
    assert b["vertex_off"].tolist() == [0, 6] and b["edge_off"].tolist() == [0, 5] and b["ref_path"].tolist() == [0, 1, 2, 3, 4, 5]
