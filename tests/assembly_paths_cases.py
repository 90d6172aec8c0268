"""The graphs tests/test_assembly_paths_hip.py runs through phmm_assembly_best_paths and tests/test_assembly_paths_oracle.py
through the restatement: the reference's own (tests/golden/assembly_paths_cases.json), the hand cases, and the shapes at which
the kernels take another path -- a queue, a tie set, a path or a vertex at and past one wave pass.  A graph is the
restatement's dict (tests/assembly_paths_restatement.py).  pack() lays graphs out as phmm_assembly_seqgraph writes them;
expected() gives every output array of the call from the restatement, computed once per set and shared."""
import functools
import json
import os
import random
import struct

import numpy as np

import assembly_paths_restatement as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "assembly_paths_cases.json")
PER_GRAPH = ("paths_status", "n_paths", "n_popped", "n_cycle_edges_removed", "n_cycle_vertices_removed")
OFFSETS = ("path_off", "path_edge_off", "hap_base_off")
PER_PATH = ("path_score", "path_is_ref", "path_n_edges")
OUTPUTS = PER_GRAPH + OFFSETS + PER_PATH + ("hap_off", "path_first_equal", "path_edges", "hap_bases", "edge_removed", "vertex_removed")
DEFAULT_NODES = 1 << 16


@functools.lru_cache(maxsize=None)
def golden():
    return json.load(open(GOLDEN))


def graph(vertices, edges, **ends):
    """vertices: strings or bytes; edges: (source, target, is_ref, multiplicity); ends: sources= / sinks= or source= / sink="""
    return dict(vertices=[x.encode() if isinstance(x, str) else bytes(x) for x in vertices], edges=[tuple(int(x) for x in e) for e in edges], **ends)


def from_json(g):
    return graph(g["vertices"], g["edges"], **{k: g[k] for k in ("sources", "sinks", "source", "sink") if k in g})


def with_roles(g):
    """the same graph with its one source and sink as sets (both present)"""
    if "sources" in g:
        return g
    assert R.NONE not in (g["source"], g["sink"])
    return dict(vertices=g["vertices"], edges=g["edges"], sources=[g["source"]], sinks=[g["sink"]])


def pack(graphs, status=None):
    """The arrays of a call: the dict best_paths takes and the roles (None if the graphs come with source / sink)"""
    roles = any("sources" in g for g in graphs)
    assert all(("sources" in g) == roles for g in graphs)
    vo, eo, bo, vbo, src, dst, ref, mult, bases, role, s, t = [0], [0], [0], [], [], [], [], [], [], [], [], []
    for g in graphs:
        at = 0
        for v in g["vertices"]:
            vbo.append(at)
            at += len(v)
            bases.append(np.frombuffer(v, np.uint8))
        if roles:
            role += [(v in g["sources"]) | 2 * (v in g["sinks"]) for v in range(len(g["vertices"]))]
        else:
            s.append(g["source"])
            t.append(g["sink"])
        for a, b, r, m in g["edges"]:
            src.append(a), dst.append(b), ref.append(r), mult.append(m)
        vo.append(vo[-1] + len(g["vertices"])), eo.append(eo[-1] + len(g["edges"])), bo.append(bo[-1] + at)
    u32 = lambda x: np.asarray(x, np.uint32)  # noqa: E731
    seq = dict(seq_vertex_off=u32(vo), seq_edge_off=u32(eo), seq_base_off=u32(bo), seq_vertex_base_off=u32(vbo), seq_edge_src=u32(src), seq_edge_dst=u32(dst),
               seq_edge_is_ref=np.asarray(ref, np.uint8), seq_edge_multiplicity=u32(mult),
               seq_bases=np.concatenate(bases + [np.zeros(0, np.uint8)]).astype(np.uint8))
    if not roles:
        seq.update(seq_ref_source=u32(s), seq_ref_sink=u32(t))
    if status is not None:
        seq["seq_status"] = u32(status)
    return seq, (np.asarray(role, np.uint8) if roles else None)


def from_seq(seq):
    """the graphs of a dict sequence_graph returned, for the restatement"""
    out = []
    for g in range(len(seq["seq_vertex_off"]) - 1):
        v0, v1, e0, e1 = (int(seq[n][g + d]) for n in ("seq_vertex_off", "seq_edge_off") for d in (0, 1))
        b0, b1 = int(seq["seq_base_off"][g]), int(seq["seq_base_off"][g + 1])
        at = [b0 + int(x) for x in seq["seq_vertex_base_off"][v0:v1]] + [b1]
        out.append(graph([seq["seq_bases"][at[i]:at[i + 1]].tobytes() for i in range(v1 - v0)],
                         list(zip(seq["seq_edge_src"][e0:e1], seq["seq_edge_dst"][e0:e1], seq["seq_edge_is_ref"][e0:e1], seq["seq_edge_multiplicity"][e0:e1])),
                         source=int(seq["seq_ref_source"][g]), sink=int(seq["seq_ref_sink"][g])))
    return out


def one(g, max_paths=128, max_nodes=DEFAULT_NODES, status=R.OK, heap=True):
    return R.best_paths(g, max_paths, max_nodes, status, heap)


def expected(graphs, max_paths=128, max_nodes=DEFAULT_NODES, regions=None, n_k=1, status=None):
    """every output array of one call over `graphs`, from the restatement; regions: the reference bytes per region, or None"""
    res = [one(g, max_paths, max_nodes, R.OK if status is None else status[i]) for i, g in enumerate(graphs)]
    o = dict(paths_status=[r["status"] for r in res], n_paths=[len(r["paths"]) for r in res], n_popped=[r["n_popped"] for r in res],
             n_cycle_edges_removed=[sum(1 for x in r["edge_removed"] if x) for r in res], n_cycle_vertices_removed=[sum(r["vertex_removed"]) for r in res])
    paths = [p for r in res for p in r["paths"]]
    o.update(path_off=np.cumsum([0] + o["n_paths"]), path_edge_off=np.cumsum([0] + [sum(len(p["edges"]) for p in r["paths"]) for r in res]),
             hap_base_off=np.cumsum([0] + [sum(len(p["bases"]) for p in r["paths"]) for r in res]))
    o = {k: np.asarray(v, np.uint32) for k, v in o.items()}
    o.update(path_score=np.asarray([p["score"] for p in paths], np.float64), path_is_ref=np.asarray([p["is_ref"] for p in paths], np.uint8),
             path_n_edges=np.asarray([len(p["edges"]) for p in paths], np.uint32), hap_off=np.cumsum([0] + [len(p["bases"]) for p in paths]).astype(np.uint32),
             path_edges=np.asarray([e for p in paths for e in p["edges"]], np.uint32),
             hap_bases=np.frombuffer(b"".join(p["bases"] for p in paths), np.uint8),
             edge_removed=np.asarray([x for r in res for x in r["edge_removed"]], np.uint8),
             vertex_removed=np.asarray([x for r in res for x in r["vertex_removed"]], np.uint8))
    if regions is not None:
        o["path_first_equal"] = np.asarray(R.first_equal(regions, n_k, [[p["bases"] for p in r["paths"]] for r in res]), np.uint32)
    o["census"] = set().union(*[r["census"] for r in res]) if res else set()
    return o


def score_bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def hex_score(x):
    return struct.pack(">d", x).hex()


# ---- the shapes -----------------------------------------------------------------------------------------------------------------------
def chain(n_edges, back_edge=False):
    """n_edges + 1 vertices in a row, unzipped; with back_edge the last but one points back at the first: the walk at depth n_edges"""
    edges = [(i, i + 1, 1, 1 + i % 3) for i in range(n_edges)]
    if back_edge:
        edges.append((n_edges - 1, 0, 0, 2))
    return graph(["ACGT"[i % 4] for i in range(n_edges + 1)], edges, source=0, sink=n_edges)


def star(n, distinct):
    """one vertex with n out-edges: the whole queue ties when the multiplicities are equal"""
    edges = [(0, 1 + i, 0, 1 + i if distinct else 1) for i in range(n)] + [(1 + i, n + 1, 0, 1) for i in range(n)]
    return graph(["A"] + ["ACGT"[i % 4] * (1 + i % 3) for i in range(n)] + ["T"], edges, source=0, sink=n + 1)


def tie_set(n_paths, first_difference):
    """n_paths paths of equal score whose edge lists first differ at position `first_difference`: a chain, then a fan"""
    d = first_difference
    edges = [(i, i + 1, 1, 1) for i in range(d)]
    edges += [(d, d + 1 + i, 0, 1) for i in reversed(range(n_paths))]   # (the higher mid by the lower edge: the order is the edges', not the vertices')
    edges += [(d + 1 + i, d + 1 + n_paths, 0, 1) for i in range(n_paths)]
    return graph(["ACGT"[i % 4] for i in range(d + n_paths + 2)], edges, source=0, sink=d + 1 + n_paths)


def vertex_bytes():
    """vertices of 0, 1, 64, 65 and 300 bytes on one path, and a second path around the longest"""
    lens = (1, 0, 1, 64, 65, 300, 0, 2)
    vertices = ["".join("ACGT"[(i + j) % 4] for j in range(n)) for i, n in enumerate(lens)]
    edges = [(i, i + 1, 1, 2) for i in range(len(lens) - 1)] + [(4, 6, 0, 1)]
    return graph(vertices, edges, source=0, sink=len(lens) - 1)


def bubbles(n, major=3, minor=1):
    """n bubbles in a row: 2^n paths"""
    vertices, edges = ["AC"], []
    for i in range(n):
        a = 3 * i
        vertices += ["G", "TT", "AC"]
        edges += [(a, a + 1, 1, major), (a, a + 2, 0, minor), (a + 1, a + 3, 1, major), (a + 2, a + 3, 0, minor)]
    return graph(vertices, edges, source=0, sink=3 * n)


def weight(total_over):
    """a vertex whose out-edges sum to PHMM_PATHS_MAX_WEIGHT + total_over"""
    half = R.MAX_WEIGHT // 2
    return graph(["A", "C", "G"], [(0, 1, 1, half), (0, 1, 0, half + total_over), (1, 2, 1, 1)], source=0, sink=2)


def random_graphs(n=250, seed=11, largest=60):
    """1 to `largest` vertices, sparse, a fifth of them cyclic, multiplicities from {0, 1, 2, 3, 10} to force ties, -inf and NaN; one or
    two sources and sinks as roles"""
    rng = random.Random(seed)
    out = []
    for i in range(n):
        nv = rng.randint(1, largest)
        edges = []
        for _ in range(rng.randint(0, nv + nv // 3)):
            a, b = rng.randrange(nv), rng.randrange(nv)
            if i % 5:   # four in five are acyclic: every edge runs upwards
                if a == b:
                    continue
                a, b = min(a, b), max(a, b)
            edges.append((a, b, rng.randrange(2), rng.choice((0, 1, 1, 2, 3, 10))))
        sources = sorted({0} | ({rng.randrange(nv)} if rng.random() < 0.3 else set()))
        sinks = sorted({nv - 1} | ({rng.randrange(nv)} if rng.random() < 0.3 else set()))
        out.append(graph(["".join(rng.choice("ACGT") for _ in range(rng.choice((0, 1, 1, 2, 5)))) for _ in range(nv)], edges, sources=sources, sinks=sinks))
    return out


def hand_cases():
    return [(c, from_json(c["graph"])) for c in golden()["hand"]]


def duplicates():
    """three k per region, two regions: equal paths in two graphs, a path equal to the reference, bytes that first differ at 255, 256, 257.
    Returns (graphs k-major, the regions' reference bytes, n_k)."""
    long_ = "ACGT" * 80
    def two(a, b, tail="G"):   # a bubble whose branches are the two strings
        return graph(["", a, b, tail], [(0, 1, 1, 2), (0, 2, 0, 1), (1, 3, 1, 1), (2, 3, 0, 1)], source=0, sink=3)
    flip = lambda s, at: s[:at] + ("A" if s[at] != "A" else "C") + s[at + 1:]  # noqa: E731
    region0 = [two("ACGTAC", "ACTTAC"), two("ACTTAC", "ACGGAC"), two("ACGTAC", "ACGGAC")]       # k0: the reference and a first; k1: an equal and a first; k2: both met
    region1 = [two(long_, flip(long_, 255)), two(flip(long_, 256), flip(long_, 257)), two(flip(long_, 255), flip(long_, 257))]
    graphs = [g for k in range(3) for g in (region0[k], region1[k])]
    return graphs, [b"ACGTACG", (long_ + "G").encode()], 3


@functools.lru_cache(maxsize=None)
def gpu_sets():
    """name -> (graphs, max_paths, max_nodes)"""
    G = golden()
    sets = {}
    by_degree = [from_json(G["score"]["graph"])] + [from_json(r["graph"]) for r in G["counts"]] + [from_json(r["graph"]) for r in G["basic_rows"]]
    by_degree += [from_json(r["graph"]) for r in G["two_paths"]]
    sets["golden, sets of sources and sinks"] = (by_degree, R.UNLIMITED, DEFAULT_NODES)
    sets["golden, singletons"] = ([from_json(r["graph"]) for r in G["basic_bubbles"] + G["triple_bubbles"]], R.UNLIMITED, DEFAULT_NODES)
    sets["golden, degenerate path pruning"] = ([from_json(G["degenerate"]["graph"])], 5, DEFAULT_NODES)
    for k in sorted({c["max_paths"] for c, _ in hand_cases()}):
        for roles in (False, True):
            graphs = [g for c, g in hand_cases() if c["max_paths"] == k and ("sources" in g) == roles]
            if graphs:
                sets["hand, max_paths %d%s" % (k, ", sets" if roles else "")] = (graphs, k, DEFAULT_NODES)
    sets["stars, equal"] = ([star(n, False) for n in (1, 63, 64, 65, 130)], 256, DEFAULT_NODES)
    sets["stars, distinct"] = ([star(n, True) for n in (1, 63, 64, 65, 130)], 256, DEFAULT_NODES)
    sets["tie sets"] = ([tie_set(n, d) for n in (2, 64, 65) for d in (0, 63, 64, 129)], 128, DEFAULT_NODES)
    sets["chains"] = ([chain(n) for n in (1, 63, 64, 65, 130, 1025)] + [chain(1025, True)], 128, DEFAULT_NODES)
    sets["vertex bytes"] = ([vertex_bytes()], 128, DEFAULT_NODES)
    for k in (1, 2, 128, R.UNLIMITED):
        sets["ten bubbles, max_paths %d" % k] = ([bubbles(10)], k, DEFAULT_NODES)
    enough = one(bubbles(4), 128)["n_created"]
    sets["budget exactly enough"] = ([bubbles(4), chain(3)], 128, enough)
    sets["budget one short"] = ([bubbles(4), chain(3)], 128, enough - 1)
    sets["no ends"] = ([dict(chain(3), source=R.NONE), chain(2), dict(chain(3), sink=R.NONE), graph([], [], source=R.NONE, sink=R.NONE)], 128, DEFAULT_NODES)
    sets["weights"] = ([weight(0), weight(1)], 128, DEFAULT_NODES)
    return sets


def census(sets):
    n = {q: 0 for q in R.QUIRKS}
    for graphs, k, nodes in sets.values():
        for g in graphs:
            for q in one(g, k, nodes)["census"]:
                n[q] += 1
    return n
