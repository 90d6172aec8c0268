"""The serial restatement of dangling-end recovery (tests/assembly_recover_restatement.py) held to the reference's own literals
(tests/golden/assembly_recover_cases.json: make_dangling_tails_data, make_dangling_heads_data, the two forked-ends tests,
get_bases_for_path of tests/read_threading_graph_unit_tests.rs) through the graph stage's restatement, and to one hand-derived
expectation per quirk.  CPU only.  The census fails when the GPU file's sets stop reaching a status, an extension or a conflict."""
import pytest

import assembly_prune_restatement as P
import assembly_recover_cases as C
import assembly_recover_restatement as R
from oracle import oracle

GOLDEN = C.golden()


def _cigar(x, i=0):
    return oracle.cigar_to_string([e for e in x["end_cigar"][i] if e])


def _run(g, cfg):
    return C.one(g, cfg)


@pytest.mark.parametrize("i", range(len(GOLDEN["tails"]["rows"])))
def test_make_dangling_tails_data(i):
    """tests/read_threading_graph_unit_tests.rs:497-684, k = 15 and the 40-base common prefix: the CIGAR, cigar_is_okay_to_merge,
    whether it merged, and the merge point's distance from the sink"""
    ref_end, alt_end, cigar, cigar_is_good, distance, allowed = GOLDEN["tails"]["rows"][i]
    g = C.tails_row(GOLDEN["tails"]["rows"][i])
    cfg = R.Config(ops=R.OP_TAILS, min_dangling_branch_length=4, min_matching_bases=allowed)
    x = _run(g, cfg)
    assert x["n_tails"] == 1, "exactly one non-reference sink"                      # :572-614
    sink = x["end_vertex"][0]
    status = x["end_status"][0]
    if status in (R.NO_PATH, R.LOOP, R.AT_REF_END, R.TOO_SHORT):                    # result is None (:626-628)
        assert not cigar_is_good
        return
    assert x["end_n_cigar"][0] == len(oracle.parse_cigar(cigar))
    assert _cigar(x) == "".join("%d%s" % (n, op) for n, op in _elements(cigar)[:4])  # :630-635
    assert (status != R.CIGAR_NOT_OKAY) == cigar_is_good                            # :638-641
    if cigar_is_good:
        assert status == R.MERGED or distance == -1                                 # :645-646
        if distance >= 0:                                                           # :649-660
            assert status == R.MERGED
            gr = x["graph"]
            v = sink
            for _ in range(distance):
                assert P.in_degree_of(gr, v) == 1
                v = gr.edge_endpoints(gr.edges_directed(v, False)[0])[0]
            assert P.out_degree_of(gr, v) > 1 and v == x["new_edge_src"][0]


def _elements(text):
    import re
    return [(int(n), op) for n, op in re.findall(r"(\d+)([MIDNSHP=X])", text)]


@pytest.mark.parametrize("i", range(len(GOLDEN["heads"]["rows"])))
def test_make_dangling_heads_data(i):
    """:928-1128, k = 5: the CIGAR, and a head that should be merged is merged (by merge_dangling_head where the allowed leading
    matches are >= 0, by merge_dangling_head_legacy otherwise)"""
    reference, alternate, cigar, should_be_merged, allowed = GOLDEN["heads"]["rows"][i]
    x = _run(C.heads_row(GOLDEN["heads"]["rows"][i]), R.Config(ops=R.OP_HEADS, min_dangling_branch_length=1, min_matching_bases=allowed))
    assert x["n_heads"] == 1
    assert _cigar(x) == cigar and x["end_n_cigar"][0] == len(_elements(cigar))      # :1026-1031
    assert x["end_status"][0] == R.MERGED or not should_be_merged                   # :1039
    if not should_be_merged:                                                        # (:1052: one path only: no bubble was made)
        assert x["end_status"][0] != R.MERGED


def test_forked_dangling_ends_with_suffix_code():
    """:687-782: the tail that ends in GCTAAGCCGATGGCT aligns against the OTHER read's branch; the CIGAR is okay, the capped suffix
    match is 0 and nothing is merged"""
    f = GOLDEN["forked_with_suffix_code"]
    g, cfg = C.golden_graphs()["forked_with_suffix_code"]
    x = _run(g, cfg)
    gr0 = R.Graph(g["k"], g["kmers"], g["edges"])
    assert len([v for v in gr0.node_indices() if P.out_degree_of(gr0, v) == 0]) == f["expect"]["n_sinks"]
    i = [g["kmers"][v] for v in x["end_vertex"]].index(f["sink_kmer"].encode())
    assert x["end_status"][i] == R.TOO_FEW_MATCHING and x["end_n_cigar"][i] <= 3 and x["end_cigar"][i][x["end_n_cigar"][i] - 1] & 15 == 0
    assert x["end_edge"][i] == R.NONE


def test_forked_dangling_ends():
    f = GOLDEN["forked"]
    g, cfg = C.golden_graphs()["forked"]
    gr0 = R.Graph(g["k"], g["kmers"], g["edges"])
    assert len([v for v in gr0.node_indices() if P.out_degree_of(gr0, v) == 0]) == f["expect"]["n_sinks"]
    x = _run(g, cfg)
    assert x["n_tails"] == 2 and x["end_status"][0] == R.MERGED


def test_get_bases_for_path():
    """:891-926: the suffix bytes for tails; for heads the source k-mer whole and reversed"""
    b = GOLDEN["get_bases_for_path"]
    g = C.from_region(b["sequence"], [], b["k"])
    gr = R.Graph(g["k"], g["kmers"], g["edges"])
    vertices, v = [], P.get_reference_source_vertex(gr)
    while v is not None:
        vertices.append(v)
        v = R.get_next_reference_vertex(gr, v, False, None)
    assert R.get_bases_for_path(gr, vertices, False) == b["tails"].encode()
    assert R.get_bases_for_path(gr, vertices, True) == b["heads"].encode()


@pytest.mark.parametrize("name", ["leading_deletion_correction", "whole_tail_insertion", "low_weight_edge_resets_the_path"])
def test_the_quirks_derived_by_hand(name):
    q = GOLDEN["quirks"][name]
    g, cfg = C.golden_graphs()["quirk_" + name]
    x = _run(g, cfg)
    want = q["expect"]
    assert R.STATUS_NAMES[x["end_status"][0]] == want["status"] and _cigar(x) == want["cigar"]
    if "edge_from_alt_index" in want:
        gr = R.Graph(g["k"], g["kmers"], g["edges"])
        _, alt_path = R.find_path_upwards_to_lowest_common_ancestor(gr, x["end_vertex"][0], g["factor"])
        ref_path = R.get_reference_path(gr, alt_path[0], True, R.get_heaviest_edge(gr, alt_path[1], False))
        assert (x["new_edge_src"][0], x["new_edge_dst"][0]) == (alt_path[want["edge_from_alt_index"]], ref_path[want["edge_to_ref_index"]])
        assert x["new_edge_multiplicity"] == [1] and x["new_edge_pruning_multiplicity"] == [1]


def test_an_extension_chains_new_vertices_with_the_removed_edges_multiplicity():
    """heads row 0 (AAYCGGTTACGT against XXXXXXXAACCGGTTACGT, legacy): the mismatch sits at index 5 of the strings while the
    dangling path has 4 vertices, so 3 vertices are made.  Their bytes continue the dangling source's k-mer backwards with the
    reference's bases; the chain carries the removed edge's multiplicity, the closing edge 1"""
    g, cfg = C.golden_graphs()["heads_00"]
    x = _run(g, cfg)
    assert x["n_new_vertices"] == 3 and x["n_new_edges"] == 4 and sum(x["edge_removed"]) == 1
    removed = x["edge_removed"].index(1)
    assert (g["kmers"][g["edges"][removed][0]], g["kmers"][g["edges"][removed][1]]) == (b"AAYCG", b"AYCGG")   # the dangling source's out-edge
    assert x["new_vertex_kmer"] == [b"AAYCG", b"XAAYC", b"XXAAY"]                  # sequence_to_extend = XXX + AAYCG, i = 3, 2, 1
    n = len(g["kmers"])
    assert list(zip(x["new_edge_src"], x["new_edge_dst"]))[:3] == [(n, g["edges"][removed][1]), (n + 1, n), (n + 2, n + 1)]
    assert x["new_edge_multiplicity"] == [g["edges"][removed][3]] * 3 + [1] and x["new_edge_pruning_multiplicity"] == x["new_edge_multiplicity"]
    assert x["new_edge_dst"][3] == n + 2 and g["kmers"][x["new_edge_src"][3]] == b"XXXAA"   # the closing edge comes from the reference


def test_the_conflict_graphs_depend_on_the_serial_order():
    graphs, cfg = C.gpu_sets()["conflicts"]
    fork, below = (_run(g, cfg) for g in graphs)
    assert [R.STATUS_NAMES[s] for s in fork["end_status"]] == ["merged", "no path"], fork["end_status"]
    assert [R.STATUS_NAMES[s] for s in below["end_status"]] == ["merged", "no path"], below["end_status"]


def test_an_extension_refused_by_the_index_range():
    q = GOLDEN["quirks"]["extension_refused_by_the_index_range"]
    g, cfg = C.golden_graphs()["quirk_extension_refused_by_the_index_range"]
    x = _run(g, cfg)
    assert x["n_heads"] == 1 and R.STATUS_NAMES[x["end_status"][0]] == q["expect"]["status"] and _cigar(x) == q["expect"]["cigar"]
    assert (x["end_alt_len"][0], x["end_ref_len"][0]) == (11, 14) and x["n_new_edges"] == 0 and x["n_new_vertices"] == 0 and not any(x["edge_removed"])


def test_the_two_head_arms_disagree():
    want = GOLDEN["quirks"]["legacy_and_new_head_arm_disagree"]["expect"]
    legacy, new = _run(*C.golden_graphs()["heads_11"]), _run(*C.golden_graphs()["heads_12"])
    assert R.STATUS_NAMES[legacy["end_status"][0]] == want["-1"] and R.STATUS_NAMES[new["end_status"][0]] == want["1"]
    assert new["n_new_vertices"] == want["new_vertices_at_1"]


def test_the_forked_ends_merge_the_first_tail_into_the_second():
    want = GOLDEN["forked"]["expect"]
    g, cfg = C.golden_graphs()["forked"]
    x = _run(g, cfg)
    assert [R.STATUS_NAMES[s] for s in x["end_status"]] == want["statuses"]
    gr = R.Graph(g["k"], g["kmers"], g["edges"])
    _, alt_path = R.find_path_upwards_to_lowest_common_ancestor(gr, x["end_vertex"][0], 0)
    ref_path = R.get_reference_path(gr, alt_path[0], True, R.get_heaviest_edge(gr, alt_path[1], False))
    assert len(alt_path) == 8 and len(ref_path) == 8 and not R.is_reference_node(gr, alt_path[0])
    assert (x["new_edge_src"][0], x["new_edge_dst"][0]) == (alt_path[want["edge_from_alt_index"]], ref_path[want["edge_to_ref_index"]])


@pytest.mark.parametrize("name", ["head_into_a_ring", "reference_path_into_a_ring"])
def test_walks_through_a_cycle_end(name):
    """cyclic graphs given without graph_flags: the loop check, and the two bounds that stand in for a reference that never returns"""
    h = GOLDEN["hand_graphs"][name]
    for factor, status in h["expect_by_factor"].items():
        x = _run(*C.golden_graphs()["hand_%s_factor_%s" % (name, factor)])
        assert [R.STATUS_NAMES[s] for s in x["end_status"]] == [status] and x["n_new_edges"] == 0, (name, factor)


def test_a_merge_index_past_the_reference_path():
    x = _run(*C.golden_graphs()["quirk_merge_index_past_the_reference_path"])
    assert [R.STATUS_NAMES[s] for s in x["end_status"]] == [GOLDEN["hand_graphs"]["merge_index_past_the_reference_path"]["expect"]] and _cigar(x) == "8M"
    assert x["end_ref_len"] == [8] and x["n_new_edges"] == 0


def test_the_census_of_what_the_gpu_sets_reach():
    """fails when the GPU file's sets stop reaching an end_status value, an extension, or a graph whose later end reads what an
    earlier end changed (n_rounds above 1)"""
    batch = C.random_regions()                                     # (the GPU file's batch of 200, with both of its configurations)
    n = C.census(list(C.gpu_sets().values()) + [(batch, R.Config(min_dangling_branch_length=1, min_matching_bases=mm)) for mm in (-1, 2)])
    for name, count in n.items():
        assert count > 0, (name, n)
