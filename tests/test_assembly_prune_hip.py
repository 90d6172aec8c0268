"""phmm_assembly_prune on the MI355X against the SERIAL restatement of the reference's graph pruning
(tests/assembly_prune_restatement.py), through the C ABI as lorikeet_amd.assembly binds it.  EQUALITY on every output array: it
is all integers and bytes, there are no tolerances.  The graphs come from tests/assembly_prune_cases.py;
tests/test_assembly_prune_oracle.py holds the restatement to the reference's literals and to hand-derived expectations and counts
on the CPU what the sets reach.  The module takes prune_graph from lorikeet_amd.assembly at the top: without the call every test
here fails."""
import numpy as np
import pytest

import assembly_graph_cases as G
import assembly_prune_cases as P
import assembly_prune_restatement as R
from lorikeet_amd import _lib
from lorikeet_amd.assembly import assembly_graph, prune_graph
from lorikeet_amd.engine import HipPairHMMEngine, PhmmError

pytestmark = pytest.mark.gpu
SETS = P.sets()
GRAPH_CALLS = G.calls()


@pytest.fixture(scope="module")
def eng():
    e = HipPairHMMEngine()
    yield e
    e.close()


def run(eng, graphs, **kw):
    a = P.pack(graphs)
    return prune_graph(eng, a, a["prune_factor"], ops=a["ops"], vertex_absent=a["vertex_absent"], edge_absent=a["edge_absent"], **kw)


def same(got, want, tag):
    for name in P.OUTPUTS:
        g, w = got[name], want[name]
        assert g.dtype == w.dtype and g.shape == w.shape, (tag, name, g.dtype, g.shape, w.dtype, w.shape)
        assert np.array_equal(g, w), (tag, name, np.argwhere(g != w)[:5].tolist(), g[g != w][:8], w[g != w][:8])


@pytest.mark.parametrize("name", sorted(SETS))
def test_equals_the_restatement(eng, name):
    """every graph of a set in a call of its own, then the set in one call: the hand graphs with every ops value, the trivial
    graphs, chains of 1 to 1 025 edges in both numberings, rings, the combs, graphs with absent elements"""
    graphs = SETS[name]
    for i, g in enumerate(graphs):
        same(run(eng, [g], fill=0xAB), P.expected([g]), (name, i))
    for ops in sorted({g["ops"] for g in graphs}):                  # (a call has one ops: the hand graphs name their own)
        together = [g for g in graphs if g["ops"] == ops]
        same(run(eng, together, fill=0xAB), P.expected(together), (name, "ops", ops))


def test_a_batch_of_300_graphs_each_equal_to_itself_alone_and_to_a_second_run(eng):
    graphs = P.batch()
    assert len(graphs) == 300 and max(g["n_vertices"] for g in graphs) >= 5000 and len({g["factor"] for g in graphs}) > 3
    first, again = run(eng, graphs, fill=0xAB), run(eng, graphs, fill=0xCD)
    same(first, P.expected(graphs), "batch")
    for name in P.OUTPUTS:
        assert first[name].tobytes() == again[name].tobytes(), name
    a = P.pack(graphs)
    for i, g in enumerate(graphs):
        alone = run(eng, [g])
        for name in P.PER_GRAPH:
            assert first[name][i] == alone[name][0], (i, name)
        for name, off in (("edge_chain", "edge_off"), ("edge_state", "edge_off"), ("vertex_state", "vertex_off")):
            assert first[name][a[off][i]:a[off][i + 1]].tobytes() == alone[name].tobytes(), (i, name)


def test_chains_then_connect_through_the_masks_equals_one_call_with_both(eng):
    graphs = P.with_ops([g for g in P.batch(60, seed=83) + SETS["hand"] if g["vertex_absent"] is None], P.ALL)
    a = P.pack(graphs)
    both = run(eng, graphs)
    first = prune_graph(eng, a, a["prune_factor"], ops=_lib.PHMM_PRUNE_OP_CHAINS)
    gone = _lib.PHMM_PRUNE_ABSENT | _lib.PHMM_PRUNE_REMOVED_CHAINS
    second = prune_graph(eng, a, a["prune_factor"], ops=_lib.PHMM_PRUNE_OP_CONNECT, vertex_absent=(first["vertex_state"] & gone) != 0,
                         edge_absent=(first["edge_state"] & gone) != 0)
    for name in ("graph_flags", "n_vertices_left", "n_edges_left", "ref_source", "ref_sink"):
        assert np.array_equal(second[name], both[name]), name
    for name in ("n_chains", "n_chains_removed", "edge_chain"):
        assert np.array_equal(first[name], both[name]), name
    merged = lambda name: first[name] & _lib.PHMM_PRUNE_REMOVED_CHAINS | second[name] & ~np.uint8(_lib.PHMM_PRUNE_ABSENT)  # noqa: E731
    assert np.array_equal(merged("vertex_state"), both["vertex_state"]) and np.array_equal(merged("edge_state"), both["edge_state"])


@pytest.mark.parametrize("name", sorted(GRAPH_CALLS))
def test_the_graphs_of_the_graph_stage_with_factors_0_to_3(eng, name):
    """assembly_graph -> prune_graph: the dict of the one goes into the other as it is"""
    c = GRAPH_CALLS[name]
    raw = assembly_graph(eng, [(g["ref"], g["reads"]) for g in c["regions"]], c["k"], c["min_q"], read_sample=G.samples_of(c),
                         num_pruning_samples=c["nps"], planes=False)
    for factor in range(4):
        want = P.pipeline(name, factor)
        assert raw["vertex_off"].tolist() == P.pack(want)["vertex_off"].tolist()
        same(prune_graph(eng, raw, factor, fill=0xAB), P.expected(want), (name, factor))


def test_no_graphs(eng):
    z = np.zeros(1, np.uint32)
    o = prune_graph(eng, dict(vertex_off=z, edge_off=z), 2, fill=0xAB)
    assert all(len(o[name]) == 0 for name in P.OUTPUTS)
    o = prune_graph(eng, dict(), None, fill=0xAB)   # n_graphs == 0: no array is looked at
    assert all(len(o[name]) == 0 for name in P.OUTPUTS)


# ---- PHMM_ERR_INVALID_ARG, every case the header names ---------------------------------------------------------------------------
def _arrays():
    return P.pack([P.graph(3, [(0, 1, 1, 3), (1, 2, 0, 1)]), P.graph(0, []), P.graph(2, [(1, 0, 0, 1)])])


def _refused(eng, a, part, factor="given", **kw):
    kw.setdefault("ops", P.ALL)
    with pytest.raises(PhmmError) as e:
        prune_graph(eng, a, a["prune_factor"] if factor == "given" else factor, fill=0xAB, **kw)
    assert e.value.code == _lib.PHMM_ERR_INVALID_ARG and part in str(e.value), str(e.value)
    assert str(e.value).count("phmm_assembly_prune") == 1
    for name, out in e.value.outputs.items():                      # nothing written
        assert (np.frombuffer(out.tobytes(), np.uint8) == 0xAB).all(), name


@pytest.mark.parametrize("name", ["vertex_off", "edge_off", "edge_src", "edge_dst", "edge_is_ref", "edge_pruning_multiplicity"])
def test_a_null_array_is_refused(eng, name):
    a = _arrays()
    a[name] = None
    _refused(eng, a, "a required pointer is NULL")
    assert name in eng.last_error()


def test_a_null_prune_factor_is_refused(eng):
    _refused(eng, _arrays(), "a required pointer is NULL (prune_factor)", factor=None)


@pytest.mark.parametrize("name", ["vertex_off", "edge_off"])
def test_offsets_that_do_not_start_at_0_or_decrease_are_refused(eng, name):
    a = _arrays()
    a[name] = a[name].copy()
    a[name][0] = 1
    _refused(eng, a, "%s does not start at 0" % name)
    a = _arrays()
    a[name] = a[name].copy()
    a[name][2] = a[name][1] - 1
    _refused(eng, a, "graph 1: %s decreases" % name)


@pytest.mark.parametrize("name, word", [("edge_src", "source"), ("edge_dst", "target")])
def test_an_endpoint_outside_its_graph_is_refused(eng, name, word):
    a = _arrays()
    a[name] = a[name].copy()
    a[name][2] = 2                                                 # graph 2 has two vertices; 2 is a vertex of graph 0 only
    _refused(eng, a, "graph 2: edge 0: its %s 2 reaches n_vertices (2)" % word)


def test_one_mask_without_the_other_is_refused(eng):
    a = _arrays()
    _refused(eng, a, "given together", vertex_absent=np.zeros(5, np.uint8))
    _refused(eng, a, "given together", edge_absent=np.zeros(3, np.uint8))


def test_a_present_edge_with_an_absent_endpoint_is_refused(eng):
    a = _arrays()
    for v in (1, 2):
        va = np.zeros(5, np.uint8)
        va[v] = 1
        _refused(eng, a, "graph 0: edge 1: it is present and an endpoint is absent", vertex_absent=va, edge_absent=np.array([1, 0, 0], np.uint8))
    va = np.zeros(5, np.uint8)
    va[1] = 7                                                      # any nonzero byte is absent; with both its edges absent it is fine
    o = prune_graph(eng, a, a["prune_factor"], vertex_absent=va, edge_absent=np.array([9, 1, 0], np.uint8))
    assert o["vertex_state"][1] == _lib.PHMM_PRUNE_ABSENT and o["edge_state"].tolist()[:2] == [_lib.PHMM_PRUNE_ABSENT] * 2


def test_ops_0_and_unknown_bits_are_refused(eng):
    _refused(eng, _arrays(), "ops is 0", ops=0)
    _refused(eng, _arrays(), "ops has unknown bits (4)", ops=4)
    _refused(eng, _arrays(), "ops has unknown bits (7)", ops=7)
