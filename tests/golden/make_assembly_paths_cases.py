"""Writes tests/golden/assembly_paths_cases.json: the literal graphs and expectations of the reference's
tests/graph_based_k_best_haplotype_finder_unit_tests.rs, written down as data, and the hand-derived cases of
tests/test_assembly_paths_oracle.py with their derivations.  A graph: vertices (strings), edges as (source, target, is_ref,
multiplicity) in the order the reference adds them (an edge's index is its petgraph EdgeIndex), and sources / sinks (the sets
the test passes) or source / sink (new_from_singletons).  Run from the repository root: python tests/golden/make_assembly_paths_cases.py"""
import json
import os

HERE = os.path.dirname(os.path.abspath(__file__))
NONE = 0xFFFFFFFF
UNLIMITED = 0xFFFFFFFF


def ends_by_degree(g):
    """get_sources_generic / get_sinks_generic: in-degree 0, out-degree 0"""
    n = len(g["vertices"])
    g["sources"] = [v for v in range(n) if all(e[1] != v for e in g["edges"])]
    g["sinks"] = [v for v in range(n) if all(e[0] != v for e in g["edges"])]
    return g


def add_edges(edges, start, remaining, is_ref, multiplicity):
    """BaseGraph::add_edges: a chain from `start` through `remaining`, every edge a copy of the template"""
    for nxt in remaining:
        edges.append([start, nxt, is_ref, multiplicity])
        start = nxt


def basic_path_finding(n_start, n_branches, n_end):
    """test_basic_path_finding (:198-236) with create_vertices (:238-281): `weight` runs through all three calls"""
    vertices, edges, weight = ["GTAC", "ACTG"], [], [1]

    def create(n, source, target):
        made = []
        for i in range(n):
            vertices.append("ACGT"[i])
            node = len(vertices) - 1
            made.append(node)
            if source is not None:
                edges.append([source, node, 0, weight[0]])
                weight[0] += 1
            if target is not None:
                edges.append([node, target, 0, weight[0]])
                weight[0] += 1
        return made
    starts = create(n_start, None, 0)
    create(n_branches, 0, 1)
    ends = create(n_end, 1, None)
    return dict(name="%d starts, %d branches, %d ends" % (n_start, n_branches, n_end), max_paths=UNLIMITED, n_paths=n_start * n_branches * n_end,
                graph=dict(vertices=vertices, edges=edges, sources=starts, sinks=ends))


def basic_bubble(ref_len, alt_len):
    """test_basic_bubble_data (:294-365): the alt path's CIGAR against pre + ref bubble + post"""
    vertices = ["ATGC", "A" * ref_len, "A" * (alt_len - 1) + "T", "GGGC"]
    edges = [[0, 1, 1, 10], [1, 3, 1, 10], [0, 2, 0, 5], [2, 3, 0, 5]]
    bubble = "%dD%dM" % (ref_len - alt_len, alt_len) if ref_len > alt_len else "%dM%dI" % (ref_len, alt_len - ref_len) if ref_len < alt_len else "%dM" % ref_len
    cigar = merged([(4, "M")] + parse(bubble) + [(4, "M")])
    return dict(name="bubble ref %d alt %d" % (ref_len, alt_len), graph=dict(vertices=vertices, edges=edges, source=0, sink=3), path=[2, 3],
                reference="ATGC" + "A" * ref_len + "GGGC", cigar=cigar)


def triple_bubble(ref_len, alt_len, off_ref_ending):
    """test_triple_bubble_data (:376-557) with off_ref_beginning = false, as make_triple_bubble_data_provider runs it"""
    alt = lambda c: c * (alt_len - 1) + "T"  # noqa: E731
    vertices = ["ATCGATCGATCGATCGATCG", "ATGG", "A" * ref_len, alt("A"), "TTCCT", "C" * ref_len, alt("C"), "CCCAAAAAAAAAAAA", "G" * ref_len, alt("G"), "GGCCG", "CCCC"]
    edges = [[0, 1, 0, 1], [1, 2, 1, 10], [2, 4, 1, 10], [1, 3, 0, 5], [3, 4, 0, 5], [4, 5, 1, 10], [5, 7, 1, 10], [4, 6, 0, 5], [6, 7, 0, 5], [7, 8, 1, 11],
             [8, 10, 1, 11], [7, 9, 0, 55], [9, 10, 0, 55], [10, 11, 0, 1]]
    path = [3, 4, 5, 6, 11, 12] + ([13] if off_ref_ending else [])
    bubble = "%dD%dM" % (ref_len - alt_len, alt_len) if ref_len > alt_len else "%dM%dI" % (ref_len, alt_len - ref_len) if ref_len < alt_len else "%dM" % ref_len
    # the CigarBuilder merges adjacent equal operators
    ops = [(4, "M")] + parse(bubble) + [(5, "M"), (ref_len, "M"), (15, "M")] + parse(bubble) + [(5, "M")] + ([(4, "I")] if off_ref_ending else [])
    reference = "ATGG" + "A" * ref_len + "TTCCT" + "C" * ref_len + "CCCAAAAAAAAAAAA" + "G" * ref_len + "GGCCG"
    return dict(name="triple bubble ref %d alt %d%s" % (ref_len, alt_len, ", off the reference at the end" if off_ref_ending else ""),
                graph=dict(vertices=vertices, edges=edges, source=1, sink=11 if off_ref_ending else 10), path=path, reference=reference,
                cigar=merged(ops))


def merged(ops):
    """CigarBuilder: adjacent equal operators become one element"""
    out = []
    for n, op in ops:
        if out and out[-1][1] == op:
            out[-1][0] += n
        else:
            out.append([n, op])
    return "".join("%d%s" % (n, op) for n, op in out)


def parse(cigar):
    out, n = [], ""
    for ch in cigar:
        if ch.isdigit():
            n += ch
        else:
            out.append((int(n), ch))
            n = ""
    return out


def two_paths(name, alternate, reference, vertices_end, cigars):
    """test_intra_node_insertion_deletion (:577-640) and test_hard_sw_path (:747-813): top, bot, alternate, reference; the reference
    path is best_paths[0], the alternate best_paths[1]"""
    edges = []
    add_edges(edges, 0, [3, 1], 1, 1)
    add_edges(edges, 0, [2, 1], 0, 1)
    return dict(name=name, max_paths=UNLIMITED, graph=dict(vertices=[vertices_end, vertices_end, alternate, reference], edges=edges, sources=[0], sinks=[1]),
                paths=[[0, 1], [2, 3]], reference=vertices_end + reference + vertices_end, cigars=cigars)


def degenerate():
    """test_degenerate_path_pruning_optimization (:659-745)"""
    vertices = ["T", "G", "C", "GGG", "G", "AAA", "A", "T", "CCCCCGGG", "TTTT"]
    edges = []
    add_edges(edges, 8, [1, 5], 0, 34)
    add_edges(edges, 8, [0, 3], 1, 33)
    add_edges(edges, 8, [2, 3], 0, 32)
    add_edges(edges, 1, [3], 0, 1)
    add_edges(edges, 5, [6, 9], 0, 15)
    add_edges(edges, 5, [7, 9], 0, 18)
    add_edges(edges, 3, [9], 1, 65)
    return dict(name="degenerate path pruning", max_paths=5, n_paths=5, graph=dict(vertices=vertices, edges=edges, source=8, sink=9),
                first_two_vertex_lists=[[8, 0, 3, 9], [8, 2, 3, 9]])


def counts():
    """test_cycle_remove (:84-117), test_no_source_or_sink (:119-151), test_dead_node (:153-196): the finder is built, and the sets
    keep their sizes"""
    e = lambda pairs: [[a, b, 0, 1] for a, b in pairs]  # noqa: E731
    rows = [dict(name="cycle remove", n_sources=1, n_sinks=1, graph=ends_by_degree(dict(vertices=list("ACGT"), edges=e([(0, 1), (1, 2), (2, 1), (2, 3)]))))]
    two = ends_by_degree(dict(vertices=list("AC"), edges=e([(0, 1)])))
    rows.append(dict(name="no source or sink: both", n_sources=1, n_sinks=1, graph=two))
    rows.append(dict(name="no source or sink: no source", n_sources=0, n_sinks=1, graph=dict(two, sources=[])))
    rows.append(dict(name="no source or sink: no sink", n_sources=1, n_sinks=0, graph=dict(two, sinks=[])))
    dead = dict(vertices=list("ACGTA"), edges=e([(0, 1), (1, 2), (2, 1), (1, 4), (0, 3)]))
    rows.append(dict(name="dead node: by degree", n_sources=1, n_sinks=2, graph=ends_by_degree(dict(dead))))
    rows.append(dict(name="dead node: singletons", n_sources=1, n_sinks=1, graph=dict(dead, sources=[0], sinks=[3])))
    return rows


def hand():
    """Expectations derived by hand from the lines of the reference; `steps` are the (m, T) of a path's edges: its score is the
    sum, left to right, of log10(m) - log10(T).  edge_removed: bit 0 the walk removed it, bit 1 it went with a vertex."""
    v = lambda n: ["ACGT"[i % 4] * (i + 1) for i in range(n)]  # noqa: E731
    p = lambda edges, steps, is_ref, bases: dict(edges=edges, steps=steps, is_ref=is_ref, bases=bases)  # noqa: E731
    return [
        dict(name="a cross edge goes although it closes no cycle", max_paths=128, quirks=["cross or forward edge removed", "cyclic"],
             derivation="5 <-> 6 make the graph cyclic, out of reach.  The walk from 0 takes e1 (0->2) first, newest first: 2, then 1 over e3, "
                        "then 3, whose e4 meets the sink: 3, 1 and 2 reach it.  Back at 0, e0 (0->1) finds 1 visited and goes, though 0->1 closes "
                        "no cycle.  No vertex goes; 5 and 6 are unvisited and stay.  One path is left: 0 2 1 3 4, every vertex with one present "
                        "out-edge, score 0.  Pops: the root and one per edge.",
             graph=dict(vertices=v(7), edges=[[0, 1, 1, 1], [0, 2, 0, 1], [1, 3, 1, 1], [2, 1, 0, 1], [3, 4, 1, 1], [5, 6, 0, 1], [6, 5, 0, 1]], source=0, sink=4),
             expected=dict(status=0, n_popped=5, edge_removed=[1, 0, 0, 0, 0, 0, 0], vertex_removed=[0] * 7,
                           paths=[p([1, 3, 2, 4], [[1, 1]] * 4, 0, "A" + "GGG" + "CC" + "TTTT" + "AAAAA")])),
        dict(name="a vertex goes because its only route runs through a visited child", max_paths=128, quirks=["vertex removed", "cyclic"],
             derivation="e5 (3->0) makes the graph cyclic.  From 0: e1 (0->2) first; 2 -> 3; at 3 e5 first: 0 is visited, e5 goes; e4 meets the "
                        "sink.  Back at 0, e0 leads to 1, unvisited: its only edge e3 (1->2) finds 2 visited and goes, so 1 reaches no sink through "
                        "first visits and is removed with e0 and e3 -- although 1 -> 2 -> 3 -> 4 is a route.  Left: 0 2 3 4; at 0 only e1 is present "
                        "(T = 3, m = 3), at 3 only e4 (T = 2, m = 2): score 0.",
             graph=dict(vertices=v(5), edges=[[0, 1, 0, 5], [0, 2, 1, 3], [2, 3, 1, 1], [1, 2, 0, 1], [3, 4, 1, 2], [3, 0, 0, 7]], source=0, sink=4),
             expected=dict(status=0, n_popped=4, edge_removed=[2, 0, 0, 3, 0, 1], vertex_removed=[0, 1, 0, 0, 0],
                           paths=[p([1, 2, 4], [[3, 3], [1, 1], [2, 2]], 1, "A" + "GGG" + "TTTT" + "AAAAA")])),
        dict(name="a cycle out of reach stays", max_paths=128, quirks=["cycles stay", "cyclic"],
             derivation="2 <-> 3 is cyclic; the walk from 0 meets the sink over e0 and removes nothing: the second assert.",
             graph=dict(vertices=v(4), edges=[[0, 1, 1, 1], [2, 3, 0, 1], [3, 2, 0, 1]], source=0, sink=1),
             expected=dict(status=4, n_popped=0, edge_removed=[0, 0, 0], vertex_removed=[0] * 4, paths=[])),
        dict(name="no path", max_paths=128, quirks=["no path", "cyclic"],
             derivation="0 <-> 1, the sink 2 isolated: e1 goes, 1 and 0 reach no sink: the first assert fires before anything is removed.",
             graph=dict(vertices=v(3), edges=[[0, 1, 1, 1], [1, 0, 0, 1]], source=0, sink=2),
             expected=dict(status=3, n_popped=0, edge_removed=[0, 0], vertex_removed=[0] * 3, paths=[])),
        dict(name="a sink with out-edges is not extended", max_paths=128, quirks=["sink with out-edges"],
             derivation="0 -> 1 -> 2 with the sink at 1: the path [e0] pops at the sink and is a result; nothing continues to 2.",
             graph=dict(vertices=v(3), edges=[[0, 1, 1, 1], [1, 2, 1, 1]], source=0, sink=1),
             expected=dict(status=0, n_popped=2, edge_removed=[0, 0], vertex_removed=[0] * 3, paths=[p([0], [[1, 1]], 1, "A" + "CC")])),
        dict(name="max_paths 1 never extends", max_paths=1, quirks=["K-th pop does not extend"],
             derivation="the root pops at 0: count[0] = 1 is not below 1, so no child is pushed; the queue is empty: no path, one pop.",
             graph=dict(vertices=v(4), edges=[[0, 1, 0, 3], [0, 2, 0, 1], [1, 3, 0, 1], [2, 3, 0, 1]], source=0, sink=3),
             expected=dict(status=0, n_popped=1, edge_removed=[0] * 4, vertex_removed=[0] * 4, paths=[])),
        dict(name="max_paths 2: the second pop of a vertex does not extend", max_paths=2, quirks=["K-th pop does not extend", "tie by edge list"],
             derivation="two parallel edges 0 -> 1, then 1 -> 2.  [e0] and [e1] tie at log10(1) - log10(2); [e0] is the smaller list and pops "
                        "first: count[1] = 1 < 2, [e0 e2] is pushed with the same score (+ 0).  [e0 e2] < [e1], so it pops: result 1.  [e1] pops at 1: "
                        "count[1] = 2 is not below 2: not extended.  The queue is empty: one path, four pops.",
             graph=dict(vertices=v(3), edges=[[0, 1, 0, 1], [0, 1, 1, 1], [1, 2, 1, 1]], source=0, sink=2),
             expected=dict(status=0, n_popped=4, edge_removed=[0] * 3, vertex_removed=[0] * 3, paths=[p([0, 2], [[1, 2], [1, 1]], 0, "A" + "CC" + "GGG")])),
        dict(name="max_paths 2: the search stops at two results", max_paths=2, quirks=["stops at K results"],
             derivation="three branches of multiplicity 3, 2, 1: root, [e0], [e0 e3] (result), [e1], [e1 e4] (result): two results, the loop "
                        "ends with [e2] still queued.",
             graph=dict(vertices=v(5), edges=[[0, 1, 1, 3], [0, 2, 0, 2], [0, 4, 0, 1], [1, 3, 1, 1], [2, 3, 0, 1], [4, 3, 0, 1]], source=0, sink=3),
             expected=dict(status=0, n_popped=5, edge_removed=[0] * 6, vertex_removed=[0] * 5,
                           paths=[p([0, 3], [[3, 6], [1, 1]], 1, "A" + "CC" + "TTTT"), p([1, 4], [[2, 6], [1, 1]], 0, "A" + "GGG" + "TTTT")])),
        dict(name="a tie decided by the edge list", max_paths=128, quirks=["tie by edge list"],
             derivation="the parallel edges again, unlimited in effect: [e0 e2] before [e1 e2], equal scores; the root and four paths pop.",
             graph=dict(vertices=v(3), edges=[[0, 1, 0, 1], [0, 1, 1, 1], [1, 2, 1, 1]], source=0, sink=2),
             expected=dict(status=0, n_popped=5, edge_removed=[0] * 3, vertex_removed=[0] * 3,
                           paths=[p([0, 2], [[1, 2], [1, 1]], 0, "A" + "CC" + "GGG"), p([1, 2], [[1, 2], [1, 1]], 1, "A" + "CC" + "GGG")])),
        dict(name="several sources: the vertex order, then the prefix rule", max_paths=128, quirks=["several sources", "tie of zero-edge paths", "tie by prefix", "tie by edge list"],
             derivation="sources 0 and 1 tie completely: 0 first (the contract).  It pushes [e0] at score 0, which ties with the zero-edge path "
                        "of 1: the empty list is a proper prefix and pops first, pushing [e1].  [e0] < [e1]: [e0] pops at 2 and pushes [e0 e2]; "
                        "[e0 e2] < [e1] pops: result.  [e1] pops at 2 (count 2), pushes [e1 e2]: result.  Six pops.",
             graph=dict(vertices=v(4), edges=[[0, 2, 1, 1], [1, 2, 0, 1], [2, 3, 1, 1]], sources=[0, 1], sinks=[3]),
             expected=dict(status=0, n_popped=6, edge_removed=[0] * 3, vertex_removed=[0] * 4,
                           paths=[p([0, 2], [[1, 1], [1, 1]], 1, "A" + "GGG" + "TTTT"), p([1, 2], [[1, 1], [1, 1]], 0, "CC" + "GGG" + "TTTT")])),
        dict(name="the NaN path pops first", max_paths=128, quirks=["NaN", "several sources", "vertex of 0 bytes"],
             derivation="the dummy fix-up's shape: 0 -> 1 over BaseEdgeStruct::new(true, 0, 0), vertex 1 empty; beside it a second source 2 -> 1 "
                        "of multiplicity 1.  Root 0 pops (vertex order) and pushes [e0] at 0 + (log10(0) - log10(0)) = -inf - -inf = NaN.  NaN is "
                        "greatest: [e0] pops before the zero-edge path of 2 at 0.0 and is the first result; then the root of 2, then [e1] at 0.",
             graph=dict(vertices=["ACGTACGT", "", "TT"], edges=[[0, 1, 1, 0], [2, 1, 0, 1]], sources=[0, 2], sinks=[1]),
             expected=dict(status=0, n_popped=4, edge_removed=[0, 0], vertex_removed=[0] * 3,
                           paths=[p([0], [[0, 0]], 1, "ACGTACGT"), p([1], [[1, 1]], 0, "TT")])),
        dict(name="a -inf path", max_paths=128, quirks=["-inf"],
             derivation="two parallel edges of multiplicity 0 and 2: T = 2; [e0] scores log10(0) - log10(2) = -inf, [e1] 0: [e1] first.",
             graph=dict(vertices=v(2), edges=[[0, 1, 1, 0], [0, 1, 0, 2]], source=0, sink=1),
             expected=dict(status=0, n_popped=3, edge_removed=[0, 0], vertex_removed=[0, 0],
                           paths=[p([1], [[2, 2]], 0, "A" + "CC"), p([0], [[0, 2]], 1, "A" + "CC")])),
        dict(name="source equals sink", max_paths=128, quirks=["source is a sink"],
             derivation="the zero-edge path pops at the sink: a result of the source's bytes, is_ref true, score 0; it is not extended.",
             graph=dict(vertices=v(2), edges=[[0, 1, 1, 1]], source=0, sink=0),
             expected=dict(status=0, n_popped=1, edge_removed=[0], vertex_removed=[0, 0], paths=[p([], [], 1, "A")])),
    ]


def main():
    score = ends_by_degree(dict(vertices=list("ACGTA"), edges=[[0, 1, 0, 1], [1, 2, 0, 1], [1, 3, 0, 1], [1, 4, 0, 1]]))
    data = dict(
        source="tests/graph_based_k_best_haplotype_finder_unit_tests.rs",
        score=dict(name="test_score", graph=score, max_paths=UNLIMITED, n_sources=1, n_sinks=3, bases="ACG", score=-0.47712125471966244),
        counts=counts(),
        basic_rows=[basic_path_finding(s, b, e) for s in (1, 2, 3) for b in (2, 3) for e in (1, 2, 3)],
        degenerate=degenerate(),
        two_paths=[two_paths("intra node insertion deletion", "AAACCCCC", "CCCCCGGG", "T", ["10M", "1M3I5M3D1M"]),
                   two_paths("hard sw path", "ACAGAGAGAGAGAGAGAGAGAGAGAGAGAGAGAGAGAGAGAGAGAGAGAGA", "TGTGTGTGTGTGTGACAGAGAGAGAGAGAGAGAGAGAGAGAGAGA", "NNN", ["51M", "3M6I48M"])],
        basic_bubbles=[basic_bubble(r, a) for r in (1, 5, 10) for a in (1, 5, 10)],
        triple_bubbles=[triple_bubble(r, a, e) for r in (1, 5, 10) for a in (1, 5, 10) for e in (True, False)],
        hand=hand())
    with open(os.path.join(HERE, "assembly_paths_cases.json"), "w") as f:
        json.dump(data, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
