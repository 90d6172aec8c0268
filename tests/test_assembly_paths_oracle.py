"""The serial restatement of the k-best haplotype finder (tests/assembly_paths_restatement.py) against the reference's own
literals, on the CPU: the graphs and expectations of tests/graph_based_k_best_haplotype_finder_unit_tests.rs, written down as
data in tests/golden/assembly_paths_cases.json, and hand-derived expectations, compared index for index, for every quirk of the
contract (the derivation stands beside each case in the JSON).  The heap version is held to a plain "take the maximum each
time" version over 300 random graphs, and a census fails when the sets the GPU file runs stop reaching a quirk.
tests/test_assembly_paths_hip.py holds phmm_assembly_best_paths to this restatement.  The module takes best_paths from
lorikeet_amd.assembly at the top: without the call every test here fails."""
import math

import pytest

import assembly_paths_cases as C
import assembly_paths_restatement as R
from lorikeet_amd import _lib
from lorikeet_amd.assembly import PATHS_OUTPUTS, best_paths

GOLD = C.golden()


def vertices_of(g, path):
    first = g["edges"][path["edges"][0]][0] if path["edges"] else None
    return [first] + [g["edges"][e][1] for e in path["edges"]]


def test_the_wrapper_exists_and_the_constants_agree():
    """(without phmm_assembly_best_paths' wrapper there is no call to hold to the restatement)"""
    assert callable(best_paths) and tuple(PATHS_OUTPUTS) == C.OUTPUTS
    names = ("OK", "SKIPPED", "NO_ENDS", "NO_PATH", "CYCLES_STAY", "WEIGHT_RANGE", "BUDGET", "MAX_WEIGHT", "EQUALS_REF")
    assert [getattr(_lib, "PHMM_PATHS_" + n) for n in names] == [getattr(R, n) for n in names]


def test_score():
    """test_score (:33-82): ACG scores -0.47712125471966244 at relative_eq!'s epsilon"""
    row = GOLD["score"]
    g = C.from_json(row["graph"])
    assert (len(g["sources"]), len(g["sinks"])) == (row["n_sources"], row["n_sinks"])
    x = C.one(g, row["max_paths"])
    acg = [p for p in x["paths"] if p["bases"] == row["bases"].encode()]
    assert len(x["paths"]) == 3 and len(acg) == 1
    # approx::relative_eq!(a, b, epsilon = EPSILON): |a - b| <= epsilon, or within max_relative (its default, EPSILON) of the larger
    diff = abs(acg[0]["score"] - row["score"])
    eps = 2.0 ** -52
    assert diff <= eps or diff <= max(abs(acg[0]["score"]), abs(row["score"])) * eps


@pytest.mark.parametrize("row", GOLD["counts"], ids=[r["name"] for r in GOLD["counts"]])
def test_the_finder_is_built_and_the_sets_keep_their_sizes(row):
    """test_cycle_remove, test_no_source_or_sink, test_dead_node: the constructor returns (no assert fires where the graph is
    cyclic) and the sets are what was passed"""
    g = C.from_json(row["graph"])
    assert (len(g["sources"]), len(g["sinks"])) == (row["n_sources"], row["n_sinks"])
    x = C.one(g, R.UNLIMITED)
    assert x["status"] == R.OK, x["status"]
    if not g["sources"] or not g["sinks"]:
        assert x["paths"] == []


@pytest.mark.parametrize("row", GOLD["basic_rows"], ids=[r["name"] for r in GOLD["basic_rows"]])
def test_basic_path_finding(row):
    """all 18 rows of make_basic_path_finding_data: the path count, and scores not increasing"""
    x = C.one(C.from_json(row["graph"]), row["max_paths"])
    assert len(x["paths"]) == row["n_paths"]
    scores = [p["score"] for p in x["paths"]]
    assert all(a >= b for a, b in zip(scores, scores[1:]))


def test_the_rows_are_all_there():
    assert len(GOLD["basic_rows"]) == 18 and len(GOLD["basic_bubbles"]) == 9 and len(GOLD["triple_bubbles"]) == 18 and len(GOLD["counts"]) == 6
    assert [r["cigars"] for r in GOLD["two_paths"]] == [["10M", "1M3I5M3D1M"], ["51M", "3M6I48M"]]
    assert sorted(m for r in GOLD["basic_rows"][-1:] for e in r["graph"]["edges"] for m in e[3:]) == list(range(1, 13))   # (weight runs through)


def test_degenerate_path_pruning_optimization():
    row = GOLD["degenerate"]
    g = C.from_json(row["graph"])
    x = C.one(g, row["max_paths"])
    assert len(x["paths"]) == row["n_paths"]
    assert [vertices_of(g, p) for p in x["paths"][:2]] == row["first_two_vertex_lists"]


@pytest.mark.parametrize("row", GOLD["two_paths"], ids=[r["name"] for r in GOLD["two_paths"]])
def test_the_two_path_orders(row):
    """test_intra_node_insertion_deletion and test_hard_sw_path: best_paths[0] is the reference path, [1] the alternate"""
    g = C.from_json(row["graph"])
    x = C.one(g, row["max_paths"])
    assert [p["edges"] for p in x["paths"]] == row["paths"]
    assert x["paths"][0]["bases"] == row["reference"].encode() and x["paths"][0]["is_ref"] and not x["paths"][1]["is_ref"]


@pytest.mark.parametrize("row", GOLD["basic_bubbles"] + GOLD["triple_bubbles"], ids=[r["name"] for r in GOLD["basic_bubbles"] + GOLD["triple_bubbles"]])
def test_the_bubble_rows_paths_are_found(row):
    """the path whose CIGAR the reference asserts is one the finder returns (the CIGARs themselves: the GPU file)"""
    x = C.one(C.from_json(row["graph"]), R.UNLIMITED)
    assert row["path"] in [p["edges"] for p in x["paths"]]
    assert any(p["bases"].startswith(row["reference"].encode()) for p in x["paths"])   # (the all-reference path; "CCCC" behind it off the end)


@pytest.mark.parametrize("case", GOLD["hand"], ids=[c["name"] for c in GOLD["hand"]])
def test_the_hand_derived_cases_index_for_index(case):
    x, want = C.one(C.from_json(case["graph"]), case["max_paths"]), case["expected"]
    assert x["status"] == want["status"] and x["n_popped"] == want["n_popped"]
    assert x["edge_removed"] == want["edge_removed"] and x["vertex_removed"] == want["vertex_removed"]
    assert len(x["paths"]) == len(want["paths"])
    for got, w in zip(x["paths"], want["paths"]):
        score = 0.0
        for m, t in w["steps"]:
            score = score + (R.log10(m) - R.log10(t))
        assert got["edges"] == w["edges"] and got["bases"] == w["bases"].encode() and got["is_ref"] == bool(w["is_ref"])
        assert C.hex_score(got["score"]) == C.hex_score(score if score == score else math.nan), (got["score"], score)
    for quirk in case["quirks"]:
        assert quirk in x["census"], (quirk, sorted(x["census"]))


def test_the_nan_and_the_minus_infinity_are_what_they_are_called():
    by_name = {c["name"]: C.one(g, c["max_paths"]) for c, g in C.hand_cases()}
    assert C.hex_score(by_name["the NaN path pops first"]["paths"][0]["score"]) == "7ff8000000000000"
    assert by_name["a -inf path"]["paths"][1]["score"] == -math.inf


def test_a_skipped_graph_and_a_graph_without_ends_are_empty():
    g = C.chain(3)
    assert C.one(g, status=1)["status"] == R.SKIPPED and C.one(g, status=1)["paths"] == []
    assert C.one(dict(g, sink=R.NONE))["status"] == R.NO_ENDS and C.one(dict(g, source=R.NONE))["status"] == R.NO_ENDS


def test_the_budget_and_the_weight_range():
    g = C.bubbles(4)
    n = C.one(g)["n_created"]
    assert C.one(g, max_nodes=n)["status"] == R.OK and len(C.one(g, max_nodes=n)["paths"]) == 16
    short = C.one(g, max_nodes=n - 1)
    assert short["status"] == R.BUDGET and short["paths"] == []
    assert C.one(C.weight(0))["status"] == R.OK and C.one(C.weight(1))["status"] == R.WEIGHT_RANGE


def test_the_heap_equals_taking_the_maximum_each_time():
    graphs = C.random_graphs(300, seed=3, largest=40)
    assert len(graphs) == 300
    for k in (1, 2, 16):
        for g in graphs:
            a, b = C.one(g, k), C.one(g, k, heap=False)
            assert a["status"] == b["status"] and a["n_popped"] == b["n_popped"]
            assert [(C.hex_score(p["score"]), p["edges"], p["is_ref"], p["bases"]) for p in a["paths"]] == \
                   [(C.hex_score(p["score"]), p["edges"], p["is_ref"], p["bases"]) for p in b["paths"]]


def test_the_duplicate_marks_as_derived():
    graphs, regions, n_k = C.duplicates()
    x = C.expected(graphs, regions=regions, n_k=n_k)
    # graphs k-major, two paths each (the reference branch first: multiplicity 2 against 1): path 2 * (2 k + r) + rank
    assert x["path_first_equal"].tolist() == [R.EQUALS_REF, R.NONE, R.EQUALS_REF, R.NONE,      # k 0: the reference; a first
                                              1, R.NONE, R.NONE, R.NONE,                       # k 1: region 0 meets k 0's again; region 1 two firsts
                                              R.EQUALS_REF, 5, 3, 7]                           # k 2: everything met before


def test_the_gpu_sets_reach_every_quirk():
    sets = dict(C.gpu_sets(), random=(C.random_graphs(), 16, C.DEFAULT_NODES))
    n = C.census(sets)
    assert all(n.values()), {q: c for q, c in n.items() if not c}
