"""The graphs tests/test_assembly_prune_oracle.py (CPU) and tests/test_assembly_prune_hip.py (GPU) share, and the serial
restatement's answer (tests/assembly_prune_restatement.py) in the layout of phmm_assembly_prune's outputs.  A graph is
dict(n_vertices, edges=[(source, target, is_ref, pruning multiplicity)], factor, ops, vertex_absent, edge_absent); a set is a
list of graphs that go into one call.  Hand graphs are data (tests/golden/assembly_prune_cases.json); the graphs of
assembly_graph_cases.calls() come through assembly_graph_restatement.graph."""
import json
import os
import random

import numpy as np

import assembly_graph_cases as G
import assembly_prune_restatement as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "assembly_prune_cases.json")
PER_GRAPH = ("graph_flags", "n_chains", "n_chains_removed", "n_vertices_left", "n_edges_left", "ref_source", "ref_sink")
OUTPUTS = PER_GRAPH + ("edge_chain", "edge_state", "vertex_state")
ALL = R.OP_CHAINS | R.OP_CONNECT
U32_MAX = 0xFFFFFFFF


def graph(n_vertices, edges, factor=2, ops=ALL, vertex_absent=None, edge_absent=None):
    assert (vertex_absent is None) == (edge_absent is None)
    return dict(n_vertices=n_vertices, edges=[tuple(e) for e in edges], factor=factor, ops=ops,
                vertex_absent=None if vertex_absent is None else list(vertex_absent), edge_absent=None if edge_absent is None else list(edge_absent))


def golden():
    return json.load(open(GOLDEN))


def hand():
    """name -> (graph, the expectation derived by hand)"""
    return {name: (graph(c["n_vertices"], c["edges"], c["factor"], c["ops"], c.get("vertex_absent"), c.get("edge_absent")), c["expect"])
            for name, c in golden().items()}


# ---- the smallest shapes at which the kernels can go wrong ----------------------------------------------------------------------
def line(n_edges, weight=1, special=None, reverse=False, **kw):
    """v0 -> v1 -> ... of n_edges edges; special: {edge: (is_ref, weight)}.  reverse: the same graph with its vertices and edges
    numbered from the far end, so that a sweep in index order carries a mark one edge per round"""
    edges = [(i, i + 1) + tuple((special or {}).get(i, (0, weight))) for i in range(n_edges)]
    if reverse:
        edges = [(n_edges - a, n_edges - b, r, w) for a, b, r, w in reversed(edges)]
    return graph(n_edges + 1, edges, **kw)


def ring(n, beside=None, weight=1):
    """a ring of n interior vertices; beside: a low chain of that many edges in the same graph"""
    edges = [(i, (i + 1) % n, 0, weight) for i in range(n)]
    if beside:
        edges += [(n + i, n + i + 1, 0, 1) for i in range(beside)]
    return graph(n + (beside + 1 if beside else 0), edges)


def chain_lengths():
    out = []
    for n in (1, 2, 63, 64, 65, 129, 1025):
        out += [line(n), line(n, special={n // 2: (0, 2)}), line(n, special={n // 2: (1, 1)}), line(n, reverse=True),
                line(n, weight=5, special={0: (1, 5), n - 1: (1, 5)}, reverse=True)]
    out += [line(5, factor=0), line(5, weight=U32_MAX - 1, factor=U32_MAX), line(5, weight=U32_MAX, factor=U32_MAX),
            line(5, special={2: (1, 0)}, factor=U32_MAX)]
    return out


def rings():
    out = []
    for n in (1, 2, 64, 65):
        out += [ring(n), ring(n, beside=3), ring(n, beside=70)]
    return out


def comb(n, reverse=False):
    """n branch vertices in series on the reference, a tooth on each: low (it goes), heavy (a dangling tail), or two edges long"""
    edges, nv = [], n + 1
    for i in range(n):
        edges.append((i, i + 1, 1, 5))
        if i % 3 == 2:
            edges += [(i, nv, 0, 1), (nv, nv + 1, 0, 1)]
            nv += 2
        else:
            edges.append((i, nv, 0, 1 if i % 3 == 0 else 4))
            nv += 1
    if reverse:
        edges = [(nv - 1 - a, nv - 1 - b, r, w) for a, b, r, w in reversed(edges)]
    return graph(nv, edges)


def tangled(rng, n_vertices, masks=False):
    """a reference path with bubbles, tails, heads, back edges, parallel edges, self-loops, stray components and isolated
    vertices, weights 0-4, vertices numbered at random"""
    n_ref = max(1, n_vertices // 2)
    edges = [(i, i + 1, 1, rng.randrange(0, 5)) for i in range(n_ref - 1)]
    free = list(range(n_ref, n_vertices))
    while free:
        kind, n = rng.randrange(8), min(len(free), rng.choice((1, 1, 2, 3, 9)))
        mid, free = free[:n], free[n:]
        w = lambda: rng.randrange(0, 5)  # noqa: E731
        inner = [(a, b, 0, w()) for a, b in zip(mid, mid[1:])]
        a, b = sorted((rng.randrange(n_ref), rng.randrange(n_ref)))
        if kind <= 1:     # a bubble (forwards) or a loop (backwards)
            edges += [(a, mid[0], 0, w())] + inner + [(mid[-1], b if kind == 0 else a, 0, w())]
        elif kind == 2:   # a tail
            edges += [(a, mid[0], 0, w())] + inner
        elif kind == 3:   # a head
            edges += inner + [(mid[-1], b, 0, w())]
        elif kind == 4:   # a stray chain, or stray vertices
            edges += inner if rng.random() < 0.5 else []
        elif kind == 5:   # a stray ring
            edges += inner + [(mid[-1], mid[0], 0, w())]
        elif kind == 6:   # a back edge and a parallel edge on the reference, a tail
            edges += [(b, a, 0, w()), (a, min(a + 1, n_ref - 1), 0, w()), (b, mid[0], 0, w())] + inner
        else:             # a ring with a way in from the reference
            edges += [(a, mid[0], 0, w())] + inner + [(mid[-1], mid[0], 0, w())]
    rng.shuffle(edges)
    name = list(range(n_vertices))
    rng.shuffle(name)
    edges = [(name[a], name[b], r, w) for a, b, r, w in edges]
    va = ea = None
    if masks:
        va = [int(rng.random() < 0.1) for _ in range(n_vertices)]
        ea = [int(va[a] or va[b] or rng.random() < 0.1) for a, b, _, _ in edges]
    return graph(n_vertices, edges, factor=rng.choice((0, 1, 2, 2, 2, 3, 5)), vertex_absent=va, edge_absent=ea)


def batch(n=300, seed=71, masks=False):
    """n graphs of 1 to several thousand vertices, a factor per graph"""
    rng = random.Random(seed)
    sizes = [1, 2, 3, 5000, 2500] + [rng.choice((1, 2, 3, 4, 6, 9, 17, 40, 64, 65, 130, 300)) for _ in range(n - 5)]
    rng.shuffle(sizes)
    return [tangled(rng, nv, masks) for nv in sizes]


_pipeline = {}


def pipeline(name, factor):
    """the graphs of one call of assembly_graph_cases.calls() in the call's order, k-major, from the graph stage's restatement"""
    if (name, factor) not in _pipeline:
        c = G.calls()[name]
        out = []
        for k in c["k"]:
            for reg in c["regions"]:
                x = G.one(reg, k, c["min_q"], c["nps"])
                out.append(graph(len(x["vertices"]), [(e[0], e[1], e[2], e[4]) for e in x["edges"]], factor))
        _pipeline[name, factor] = out
    return _pipeline[name, factor]


def sets():
    """name -> list of graphs: every set the GPU file runs, each graph alone and all of a set in one call"""
    out = {"hand": [g for g, _ in hand().values()], "trivial": [graph(0, []), graph(1, []), graph(2, []), graph(1, [(0, 0, 0, 1)]), graph(0, [])],
           "chain_lengths": chain_lengths(), "rings": rings(), "comb": [comb(2000), comb(2000, reverse=True), comb(7)]}
    for ops in (R.OP_CHAINS, R.OP_CONNECT):
        out["hand_ops%d" % ops] = with_ops([g for g, _ in hand().values()], ops)
    out["masks"] = batch(40, seed=73, masks=True)
    return out


def with_ops(graphs, ops):
    return [dict(g, ops=ops) for g in graphs]


# ---- the restatement's answer in the call's layout ------------------------------------------------------------------------------
_memo = {}


def one(g):
    key = (g["n_vertices"], tuple(g["edges"]), g["factor"], g["ops"], None if g["vertex_absent"] is None else (tuple(g["vertex_absent"]), tuple(g["edge_absent"])))
    if key not in _memo:
        _memo[key] = R.prune(g["n_vertices"], g["edges"], g["factor"], g["ops"], g["vertex_absent"], g["edge_absent"])
    return _memo[key]


def pack(graphs):
    """the input arrays of a call (one ops for all its graphs); the masks are given when any graph has them"""
    assert len({g["ops"] for g in graphs}) <= 1
    masks = any(g["vertex_absent"] is not None for g in graphs)
    cat = lambda rows, dt: np.asarray([x for row in rows for x in row], dt)  # noqa: E731
    a = dict(vertex_off=np.cumsum([0] + [g["n_vertices"] for g in graphs]).astype(np.uint32),
             edge_off=np.cumsum([0] + [len(g["edges"]) for g in graphs]).astype(np.uint32),
             prune_factor=np.asarray([g["factor"] for g in graphs], np.uint32), ops=graphs[0]["ops"] if graphs else ALL)
    for j, (name, dt) in enumerate((("edge_src", np.uint32), ("edge_dst", np.uint32), ("edge_is_ref", np.uint8), ("edge_pruning_multiplicity", np.uint32))):
        a[name] = cat([[e[j] for e in g["edges"]] for g in graphs], dt)
    a["vertex_absent"] = cat([g["vertex_absent"] or [0] * g["n_vertices"] for g in graphs], np.uint8) if masks else None
    a["edge_absent"] = cat([g["edge_absent"] or [0] * len(g["edges"]) for g in graphs], np.uint8) if masks else None
    return a


def expected(graphs):
    """the output arrays of a call, from the restatement"""
    xs = [one(g) for g in graphs]
    o = {name: np.asarray([x[name] for x in xs], np.uint32) for name in PER_GRAPH}
    for name, dt in (("edge_chain", np.uint32), ("edge_state", np.uint8), ("vertex_state", np.uint8)):
        o[name] = np.asarray([v for x in xs for v in x[name]], dt)
    return o


REQUIRED_BRANCHES = ("chain ends: no out-edge", "chain ends: several out-edges", "chain ends: several in-edges", "chain end seen before",
                     "chain removed", "chain kept", "orphan removed", "an edge in no chain", "orphan kept: the only vertex",
                     "a reference edge protects a low chain", "cycle", "no ref ends", "dangling tail", "dangling head",
                     "one node: source and sink", "connect removes")


def census(all_sets):
    """which branches of the restatement the sets reach: a name -> count dict (tests/test_assembly_prune_oracle.py fails on a 0),
    with what only the shapes show: a graph past one pass of 256 lanes, absent elements, every ops value"""
    n = {name: 0 for name in REQUIRED_BRANCHES}
    n.update(more_edges_than_lanes=0, absent_elements=0, ops_1=0, ops_2=0, ops_3=0, pruning_removes_a_cycle=0)
    for graphs in all_sets:
        for g in graphs:
            x = one(g)
            for name in x["census"]:
                n[name] += 1
            n["more_edges_than_lanes"] += len(g["edges"]) > 256
            n["absent_elements"] += g["vertex_absent"] is not None and any(g["vertex_absent"]) and any(g["edge_absent"])
            n["ops_%d" % g["ops"]] += 1
            if g["ops"] & R.OP_CHAINS and g["factor"] and not x["graph_flags"] & R.HAS_CYCLE:
                n["pruning_removes_a_cycle"] += bool(one(dict(g, factor=0))["graph_flags"] & R.HAS_CYCLE)
    return n
