"""The graphs the sequence-graph tests run (tests/test_assembly_seqgraph_oracle.py on the CPU, tests/test_assembly_seqgraph_hip.py on
the GPU): the rows of the reference's make_linear_zip_data and the hand-derived cases of tests/golden/assembly_seqgraph_cases.json,
chains at the edges of a wave and of a workgroup, many chains and many zip starts on one graph, chain into chain, random graphs;
the arrays of a call for them, and the restatement's answer in the call's layout."""
import json
import os
import random

import numpy as np

import assembly_seqgraph_restatement as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "assembly_seqgraph_cases.json")
PER_GRAPH = ("seq_status", "n_seq_vertices", "n_seq_edges", "n_seq_bases", "n_chains_zipped", "n_removed_clean", "n_removed_unconnected",
             "seq_ref_source", "seq_ref_sink")
OFFSETS = ("seq_vertex_off", "seq_edge_off", "seq_base_off")
PER_VERTEX = ("seq_vertex_base_off", "seq_vertex_first", "seq_vertex_n_merged")
PER_EDGE = ("seq_edge_src", "seq_edge_dst", "seq_edge_is_ref", "seq_edge_multiplicity")
OUTPUTS = PER_GRAPH + OFFSETS + PER_VERTEX + PER_EDGE + ("seq_bases", "vertex_to_seq")
BASES = (b"A", b"C", b"G", b"T", b"TT", b"GG", b"CC", b"AA")   # the eight repeating sequences of the reference's chains
# what the GPU sets must reach (census): every quirk of the contract
QUIRKS = ("zip: a reference break", "zip: last -> first", "zip: chain into chain, the source merged first", "zip: chain into chain, the target merged first",
          "zip: an interior vertex stays (a ring, or behind a reference break)", "connectivity: a weakly connected vertex goes",
          "connectivity: no reference source", "one node", "clean removes in front of the source", "clean removes behind the sink", "clean orphans a vertex",
          "clean: an end is missing", "reference fails in front of the source: it panics in this order",
          "reference fails in front of the source: it survives in this order", "reference fails behind the sink: it panics in this order",
          "a source vertex carries k bytes", "a recovery-made vertex", "an orphan behind the zip", "skipped")


def golden():
    return json.load(open(GOLDEN))


def graph(k, kmers, edges, vertex_absent=None, edge_absent=None, n_new=0, flags=0):
    """kmers: the k bytes of every vertex; edges: (source, target, is_ref, multiplicity); n_new: how many of the last vertices are
    recovery's (their bytes travel in new_vertex_kmer); flags: phmm_assembly_prune's graph_flags"""
    kmers = [x.encode() if isinstance(x, str) else bytes(x) for x in kmers]
    assert (vertex_absent is None) == (edge_absent is None) and all(len(x) == k for x in kmers) and n_new <= len(kmers)
    return dict(k=k, kmers=kmers, edges=[tuple(int(x) for x in e) for e in edges], n_new=n_new, flags=flags,
                vertex_absent=None if vertex_absent is None else [int(x) for x in vertex_absent],
                edge_absent=None if edge_absent is None else [int(x) for x in edge_absent])


def hand_graphs():
    return {c["name"]: graph(c["k"], c["kmers"], c["edges"], n_new=c["n_new"]) for c in golden()["hand"]}


def zip_row_graph(row, k=1):
    """a row of make_linear_zip_data as an input graph: possible where every vertex has one byte.  A vertex of in-degree 0 carries
    its k bytes, so with k = 1 the conversion gives the row's own vertices"""
    assert all(len(v) == 1 for v in row["vertices"])
    return graph(k, row["vertices"], row["edges"])


def _dna(rng, n):
    return bytes(rng.choice(b"ACGT") for _ in range(n))


def chain(n, k=3, against=False, ref=True, seed=7):
    """n vertices in one chain on reference edges, numbered along the chain or against it"""
    rng = random.Random(seed * 1000 + n)
    order = list(range(n))[::-1] if against else list(range(n))
    kmers = [_dna(rng, k) for _ in range(n)]
    return graph(k, kmers, [(order[i], order[i + 1], int(ref), 1 + i % 7) for i in range(n - 1)])


def bubbles(n_chains, length=3, k=5, seed=11):
    """a reference path S -> J1 -> J2 ... with, between each pair of junctions, a reference chain and a non-reference chain of
    `length` vertices: 2 x n_chains zip starts, all merged"""
    rng = random.Random(seed + n_chains)
    kmers, edges = [_dna(rng, k)], []
    prev = 0
    for _ in range(n_chains):
        tops = []
        for is_ref in (1, 0):
            at = prev
            for _ in range(length):
                kmers.append(_dna(rng, k))
                edges.append((at, len(kmers) - 1, is_ref, rng.randrange(1, 50)))
                at = len(kmers) - 1
            tops.append(at)
        kmers.append(_dna(rng, k))
        j = len(kmers) - 1
        edges += [(tops[0], j, 1, 3), (tops[1], j, 0, 2)]
        prev = j
    return graph(k, kmers, edges)


def star(n_starts, k=4, seed=13):
    """S -> T on a reference edge and a non-reference one, and n_starts chains of two S -> a_i -> b_i -> T: n_starts zip starts whose merged
    vertices all hang on S and T, so S's out-edges and T's in-edges are all re-created"""
    rng = random.Random(seed + n_starts)
    kmers, edges = [_dna(rng, k), _dna(rng, k)], [(0, 1, 1, 9), (0, 1, 0, 8)]
    for i in range(n_starts):
        kmers += [_dna(rng, k), _dna(rng, k)]
        a = len(kmers) - 2
        edges += [(0, a, 0, 1 + i % 5), (a, a + 1, 0, 2), (a + 1, 1, 0, 3 + i % 3)]
    return graph(k, kmers, edges)


def random_graphs(n=200, seed=43, largest=3000):
    """mostly small, a few up to `largest` vertices: runs along shuffled indices with reference and non-reference stretches, extra edges,
    sometimes masks, sometimes parallel edges and self-loops"""
    rng = random.Random(seed)
    out = []
    for i in range(n):
        nv = 1 + (i * (largest - 1)) // 4 if i < 5 else rng.randrange(1, rng.choice([4, 8, 16, 40, 90]))
        k = rng.choice([1, 3, 5, 11])
        kmers = [_dna(rng, k) for _ in range(nv)]
        perm = list(range(nv))
        if rng.random() < 0.7:
            rng.shuffle(perm)
        edges, is_ref = [], rng.random() < 0.5
        for j in range(nv - 1):
            if rng.random() < 0.06:
                is_ref = not is_ref
            if rng.random() < 0.93:
                edges.append((perm[j], perm[j + 1], int(is_ref), rng.randrange(1, 9)))
        for _ in range(rng.randrange(0, max(2, nv // 6))):
            edges.append((rng.randrange(nv), rng.randrange(nv), int(rng.random() < 0.15), rng.randrange(1, 9)))
        if rng.random() < 0.5:
            rng.shuffle(edges)
        va = ea = None
        if rng.random() < 0.3:
            va = [int(rng.random() < 0.05) for _ in range(nv)]
            ea = [int(rng.random() < 0.05 or va[e[0]] or va[e[1]]) for e in edges]
        out.append(graph(k, kmers, edges, va, ea, n_new=rng.randrange(0, min(nv, 3) + 1) if rng.random() < 0.3 else 0))
    return out


def compacted(g):
    """the same graph without its absent elements, renumbered by hand"""
    va, ea = g["vertex_absent"], g["edge_absent"]
    new = {}
    for v in range(len(g["kmers"])):
        if not va[v]:
            new[v] = len(new)
    return graph(g["k"], [g["kmers"][v] for v in new], [(new[a], new[b], r, m) for e, (a, b, r, m) in enumerate(g["edges"]) if not ea[e]]), new


# ---- a call: its arrays, and the restatement's answer in the call's layout ----------------------------------------------------------
def pack(graphs):
    """(regions, graph, applied, slots): the arguments of lorikeet_amd.assembly.sequence_graph for these graphs in one call.  The layout
    is k-major: slot (k index, region r) holds graph r where its k is that k, and an empty graph elsewhere; slots[r] is graph r's
    slot.  A graph's region is its raw vertices' k-mers one behind the other; its new vertices' k-mers are rows of new_vertex_kmer"""
    ks = sorted({g["k"] for g in graphs})
    k_max = max(ks) if ks else 0
    n = len(graphs)
    regions = [(b"".join(g["kmers"][:len(g["kmers"]) - g["n_new"]]), []) for g in graphs]
    vertex_off, edge_off, new_off, rows = [0], [0], [0], []
    cols = {name: [] for name in ("vertex_seq", "vertex_pos", "edge_src", "edge_dst", "edge_is_ref", "edge_multiplicity", "vertex_absent", "edge_absent", "flags")}
    slots = [ks.index(g["k"]) * n + r for r, g in enumerate(graphs)]
    for k in ks:
        for g in graphs:
            mine = g["k"] == k
            nv, edges, n_new = (len(g["kmers"]), g["edges"], g["n_new"]) if mine else (0, [], 0)
            cols["vertex_seq"] += [0] * (nv - n_new)
            cols["vertex_pos"] += [v * k for v in range(nv - n_new)]
            rows += [list(km) + [0] * (k_max - k) for km in g["kmers"][nv - n_new:nv]] if mine else []
            for j, name in enumerate(("edge_src", "edge_dst", "edge_is_ref", "edge_multiplicity")):
                cols[name] += [e[j] for e in edges]
            cols["vertex_absent"] += (g["vertex_absent"] or [0] * nv) if mine else []
            cols["edge_absent"] += (g["edge_absent"] or [0] * len(edges)) if mine else []
            cols["flags"].append(g["flags"] if mine else 0)
            vertex_off.append(vertex_off[-1] + nv)
            edge_off.append(edge_off[-1] + len(edges))
            new_off.append(new_off[-1] + n_new)
    arr = lambda name, dt: np.asarray(cols[name], dt)  # noqa: E731
    gd = dict(k=np.asarray(ks, np.uint32), vertex_seq=arr("vertex_seq", np.uint32), vertex_pos=arr("vertex_pos", np.uint32))
    applied = dict(vertex_off=np.asarray(vertex_off, np.uint32), edge_off=np.asarray(edge_off, np.uint32), edge_src=arr("edge_src", np.uint32),
                   edge_dst=arr("edge_dst", np.uint32), edge_is_ref=arr("edge_is_ref", np.uint8), edge_multiplicity=arr("edge_multiplicity", np.uint32),
                   vertex_absent=arr("vertex_absent", np.uint8), edge_absent=arr("edge_absent", np.uint8), graph_flags=arr("flags", np.uint32),
                   new_vertex_off=np.asarray(new_off, np.uint32), new_vertex_kmer=np.asarray(rows, np.uint8).reshape(-1, k_max))
    return regions, gd, applied, slots


_memo = {}


def one(g):
    key = (g["k"], tuple(g["kmers"]), tuple(g["edges"]), g["flags"], None if g["vertex_absent"] is None else (tuple(g["vertex_absent"]), tuple(g["edge_absent"])))
    if key not in _memo:
        x = R.sequence_graph(len(g["kmers"]), g["edges"], g["kmers"], g["vertex_absent"], g["edge_absent"], g["flags"])
        if g["n_new"]:
            x["census"].add("a recovery-made vertex")
        _memo[key] = x
    return _memo[key]


def expected(graphs):
    """the output arrays of the call pack(graphs) describes, from the restatement"""
    ks = sorted({g["k"] for g in graphs})
    xs = [one(g) if g["k"] == k else R.empty(R.OK, 0) for k in ks for g in graphs]
    o = {name: np.asarray([x[name] for x in xs], np.uint32) for name in PER_GRAPH}
    for off, count in zip(OFFSETS, ("n_seq_vertices", "n_seq_edges", "n_seq_bases")):
        o[off] = np.cumsum([0] + [x[count] for x in xs]).astype(np.uint32)
    for name in PER_VERTEX + PER_EDGE + ("vertex_to_seq",):
        o[name] = np.asarray([v for x in xs for v in x[name]], np.uint8 if name == "seq_edge_is_ref" else np.uint32)
    o["seq_bases"] = np.frombuffer(b"".join(x["seq_bases"] for x in xs), np.uint8)
    return o


def gpu_sets():
    """name -> graphs: every set the GPU file runs, each graph alone and all of a set in one call"""
    g = golden()
    out = {"golden_rows": [zip_row_graph(r) for r in g["zip_rows"] if all(len(v) == 1 for v in r["vertices"])],
           "hand": list(hand_graphs().values())}
    skipped = [dict(out["hand"][0], flags=1), dict(out["hand"][1], flags=2)]
    out["hand"] += skipped
    out["chains"] = [chain(n, against=a) for n in (1, 2, 63, 64, 65, 129, 255, 256, 257, 1025) for a in (False, True)]
    out["source_bytes"] = [chain(n, k=k) for k in (3, 65) for n in (1, 2, 62, 64, 66, 127, 130)]
    out["many_chains"] = [bubbles(1), bubbles(32), bubbles(33), star(64), star(65), star(300)]
    return out


def census(sets):
    """how often the sets reach each quirk of the contract"""
    n = {q: 0 for q in QUIRKS}
    for graphs in sets.values():
        for g in graphs:
            for c in one(g)["census"]:
                if c in n:
                    n[c] += 1
    return n
