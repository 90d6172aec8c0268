"""The serial restatement of the reference's graph pruning (tests/assembly_prune_restatement.py) held to the reference's own
literals and to expectations derived by hand from the cited lines, one per quirk (tests/golden/assembly_prune_cases.json); a
census of what the GPU sets (tests/assembly_prune_cases.py) reach; and the binding of phmm_assembly_prune in the library, the
header, the ctypes table and the Rust declarations.  CPU only.
Line numbers: C = src/graphs/chain_pruner.rs, L = src/graphs/low_weight_chain_pruner.rs, B = src/graphs/base_graph.rs."""
import os
import re

import pytest

import assembly_graph_cases as G
import assembly_graph_restatement as GR
import assembly_prune_cases as P
import assembly_prune_restatement as R
from lorikeet_amd import _lib
from lorikeet_amd.assembly import prune_graph  # noqa: F401  (the binding this file is about: without it nothing here runs)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HAND = P.hand()


def test_the_export_is_in_the_library_the_binding_and_the_rust_declarations():
    lib = _lib.load()
    ffi = open(os.path.join(ROOT, "integration", "hip_ffi.rs")).read()
    header = open(os.path.join(ROOT, "include", "phmm.h")).read()
    n = "phmm_assembly_prune"
    assert getattr(lib, n) is not None
    args = next(a for name, _, a in _lib.SYMBOLS if name == n)
    decl = re.search(r"pub fn %s\s*\(([^)]*)\)" % n, ffi, re.S).group(1)
    c_decl = re.search(r"\bint %s\(([^)]*)\)" % n, header, re.S).group(1)
    assert len(args) == len([x for x in decl.split(",") if x.strip()]) == len(c_decl.split(",")) == 22
    names = ("OP_CHAINS", "OP_CONNECT", "HAS_CYCLE", "NO_REF_ENDS", "ABSENT", "REMOVED_CHAINS", "REMOVED_CONNECT", "DANGLING_TAIL", "DANGLING_HEAD")
    for name in names:
        value = int(re.search(r"#define PHMM_PRUNE_%s (\d+)u?\b" % name, header).group(1))
        assert getattr(_lib, "PHMM_PRUNE_" + name) == value == getattr(R, name), name
        assert re.search(r"pub const PHMM_PRUNE_%s: \w+ = %d;" % (name, value), ffi), name
    backend = open(os.path.join(ROOT, "integration", "hip_backend.rs")).read()
    assert "pub fn assembly_prune(" in backend and "phmm_assembly_prune(" in backend
    import tools.source_hash as SH
    assert {"phmm_prune_internal.hpp", "phmm_prune_kernels.hip"} <= set(SH.KERNEL_SOURCES["prune"])
    assert "prune=%s" % SH.source_hash("prune") in lib.phmm_build_info().decode()
    import lorikeet_amd
    assert lorikeet_amd.prune_graph is lorikeet_amd.assembly.prune_graph


# ---- the reference's own literals --------------------------------------------------------------------------------------------
def test_the_doc_comment_of_the_low_weight_pruner():
    """L:10-11"""
    gone, stays = (R.prune(4, [(0, 1, 0, 1), (1, 2, 0, m, ), (2, 3, 0, 1)], 2, R.OP_CHAINS) for m in (1, 2))
    assert gone["n_chains"] == stays["n_chains"] == 1
    assert gone["n_chains_removed"] == 1 and gone["n_edges_left"] == 0 and gone["edge_state"] == [R.REMOVED_CHAINS] * 3
    assert stays["n_chains_removed"] == 0 and stays["n_edges_left"] == 3 and stays["edge_state"] == [0] * 3


@pytest.mark.parametrize("weight", [1, 2, 3])
@pytest.mark.parametrize("factor", [1, 2, 3, 4])
@pytest.mark.parametrize("is_ref", [True, False])
def test_the_isolated_chain_of_the_references_unit_tests(weight, factor, is_ref):
    """chain_pruner_unit_tests.rs:86-117: A -> C -> G with one weight is ONE chain (find_all_chains, :56); with the low-weight
    pruner it goes exactly when weight < factor and it is not reference (the test's own n_expected, :90-94)"""
    edges = [(0, 1, int(is_ref), weight), (1, 2, int(is_ref), weight)]
    g = R.StableGraph(3, edges)
    chains = R.find_all_chains(g, set())
    assert len(chains) == 1 and chains[0] == (2, [0, 1])
    assert R.needs_pruning(g, chains[0], factor) == (weight < factor and not is_ref)
    x = R.prune(3, edges, factor, R.OP_CHAINS)
    assert x["n_vertices_left"] == (0 if weight < factor and not is_ref else 3)


def test_cycles_in_graph():
    """the graph stage's cycle region: a cycle at the small k, none at the large one, nothing pruned (factor 0)"""
    reg, c = G.cycle_region()
    for k, want in ((c["k_with_cycle"], R.HAS_CYCLE), (c["k_without_cycle"], 0)):
        x = GR.graph(reg["ref"], reg["reads"], k)
        y = R.prune(len(x["vertices"]), [(e[0], e[1], e[2], e[4]) for e in x["edges"]], 0, R.OP_CHAINS)
        assert y["graph_flags"] & R.HAS_CYCLE == want and y["n_chains_removed"] == 0 and y["n_edges_left"] == len(x["edges"])


# ---- one hand-derived expectation per quirk (the derivations are the notes beside the data) ---------------------------------------
@pytest.mark.parametrize("name", sorted(HAND))
def test_hand_derived(name):
    g, want = HAND[name]
    got = P.one(g)
    assert {key: got[key] for key in want} == want


def test_find_chain_stops_where_it_started():
    """C:108: on a ring the walk comes back to the first vertex and ends there, with every edge of the ring once.  find_all_chains
    never starts on such an edge (its starts are sources and chain ends), so the pruner leaves rings alone"""
    g = R.StableGraph(3, [(0, 1, 0, 1), (1, 2, 0, 1), (2, 0, 0, 1)])
    census = set()
    assert R.find_chain(g, 1, census) == (1, [1, 2, 0]) and census == {"chain ends: back at its start"}
    assert not R.find_all_chains(g, set())
    x = R.prune(3, [(0, 1, 0, 1), (1, 2, 0, 1), (2, 0, 0, 1)], 2, P.ALL)
    assert x["edge_chain"] == [R.NONE] * 3 and x["n_edges_left"] == 3 and x["graph_flags"] == R.HAS_CYCLE | R.NO_REF_ENDS


def test_edges_directed_walks_from_the_newest_edge():
    """petgraph's adjacency lists grow at the head: the chains of a branch vertex come out newest first (C:69)"""
    g = R.StableGraph(4, [(0, 1, 0, 1), (0, 2, 0, 1), (0, 3, 0, 1)])
    assert g.edges_directed(0, True) == [2, 1, 0]
    assert [c[1] for c in R.find_all_chains(g, set())] == [[2], [1], [0]]


def test_chains_then_connect_through_the_masks_is_one_call_with_both():
    """what the absent masks are for: the caller changes the graph between the two steps (dangling-end recovery); unchanged, the
    two calls give what one call gives"""
    for g in [h for h, _ in HAND.values() if h["vertex_absent"] is None] + P.batch(30, seed=79):
        both = P.one(dict(g, ops=P.ALL))
        first = P.one(dict(g, ops=R.OP_CHAINS))
        gone = R.ABSENT | R.REMOVED_CHAINS
        second = P.one(dict(g, ops=R.OP_CONNECT, vertex_absent=[int(bool(s & gone)) for s in first["vertex_state"]],
                            edge_absent=[int(bool(s & gone)) for s in first["edge_state"]]))
        for name in ("graph_flags", "n_vertices_left", "n_edges_left", "ref_source", "ref_sink"):
            assert second[name] == both[name], name
        for name in ("vertex_state", "edge_state"):  # (what the first call removed is absent in the second)
            assert [bool(s & (gone | R.REMOVED_CONNECT)) for s in both[name]] == [bool(s & (gone | R.REMOVED_CONNECT)) for s in second[name]], name
        dangling = R.DANGLING_TAIL | R.DANGLING_HEAD
        assert [s & dangling for s in both["vertex_state"]] == [s & dangling for s in second["vertex_state"]]


# ---- what the GPU sets reach ---------------------------------------------------------------------------------------------------
def test_the_gpu_sets_reach_every_branch():
    n = P.census(list(P.sets().values()) + [P.batch()])
    assert all(v > 0 for v in n.values()), n


def test_the_layout_of_the_packed_and_expected_arrays():
    graphs = [P.graph(2, [(0, 1, 1, 3)]), P.graph(0, []), P.graph(3, [(2, 1, 0, 1), (1, 0, 0, 1)], factor=7, vertex_absent=[0, 0, 0], edge_absent=[0, 1])]
    a, o = P.pack(graphs), P.expected(graphs)
    assert a["vertex_off"].tolist() == [0, 2, 2, 5] and a["edge_off"].tolist() == [0, 1, 1, 3] and a["prune_factor"].tolist() == [2, 2, 7]
    assert a["edge_src"].tolist() == [0, 2, 1] and a["edge_dst"].tolist() == [1, 1, 0] and a["edge_is_ref"].tolist() == [1, 0, 0]
    assert a["vertex_absent"].tolist() == [0] * 5 and a["edge_absent"].tolist() == [0, 0, 1]
    assert o["edge_chain"].tolist() == [0, 0, R.NONE] and o["n_chains"].tolist() == [1, 0, 1] and len(o["vertex_state"]) == 5
