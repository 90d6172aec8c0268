"""The graphs tests/test_assembly_recover_oracle.py (CPU) and tests/test_assembly_recover_hip.py (GPU) share, and the serial
restatement's answer (tests/assembly_recover_restatement.py) in the layout of phmm_assembly_recover's outputs.  A graph is
dict(k, kmers=[bytes per vertex], edges=[(source, target, is_ref, multiplicity, pruning multiplicity)], factor, vertex_absent,
edge_absent).  Graphs of real regions come through assembly_graph_restatement (the raw graph) and assembly_prune_restatement
(CHAINS makes the masks); hand graphs are threaded here from sequences whose k-mers are all different.  For a call every graph
becomes a region of its own whose reference is its vertices' k-mers one behind the other, so vertex_seq = 0 and vertex_pos = v * k
name any bytes a test wants."""
import json
import os
import random

import numpy as np

import assembly_graph_cases as G
import assembly_prune_restatement as P
import assembly_recover_restatement as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "assembly_recover_cases.json")
PER_GRAPH = ("n_tails", "n_tails_recovered", "n_heads", "n_heads_recovered", "n_new_edges", "n_new_vertices")
OFFSETS = ("end_off", "new_edge_off", "new_vertex_off")
PER_END = ("end_vertex", "end_kind", "end_status", "end_alt_len", "end_ref_len", "end_n_cigar", "end_cigar", "end_edge")
PER_EDGE = ("new_edge_src", "new_edge_dst", "new_edge_multiplicity", "new_edge_pruning_multiplicity")
OUTPUTS = PER_GRAPH + OFFSETS + PER_END + PER_EDGE + ("new_vertex_kmer", "edge_removed")   # (n_rounds: the schedule's, not the reference's)
GONE = P.ABSENT | P.REMOVED_CHAINS | P.REMOVED_CONNECT


def golden():
    return json.load(open(GOLDEN))


def graph(k, kmers, edges, factor=0, vertex_absent=None, edge_absent=None):
    assert (vertex_absent is None) == (edge_absent is None) and all(len(x) == k for x in kmers)
    return dict(k=k, kmers=[bytes(x) for x in kmers], edges=[tuple(int(x) for x in e) for e in edges], factor=factor,
                vertex_absent=None if vertex_absent is None else [int(x) for x in vertex_absent],
                edge_absent=None if edge_absent is None else [int(x) for x in edge_absent])


def from_region(ref, reads, k, factor=0, chains=False, min_q=10, nps=1, samples=None):
    """the raw graph of a region as the graph stage's restatement builds it; chains: what prune_low_weight_chains removes is absent"""
    reg = G.region(ref, reads, samples)
    x = G.one(reg, k, min_q, nps)
    seqs = [reg["ref"]] + [b for b, _ in reg["reads"]]
    kmers = [seqs[s][pos:pos + k] for s, pos, _ in x["vertices"]]
    va = ea = None
    if chains:
        pr = P.prune(len(kmers), [(e[0], e[1], e[2], e[4]) for e in x["edges"]], factor, P.OP_CHAINS)
        va, ea = [int(bool(s & GONE)) for s in pr["vertex_state"]], [int(bool(s & GONE)) for s in pr["edge_state"]]
    return graph(k, kmers, x["edges"], factor, va, ea)


def threaded(k, ref, alts, factor=0):
    """a graph threaded by hand: a vertex per distinct k-mer in order of appearance (the reference first), an edge per pair of
    neighbours; alts: sequences or (sequence, weight).  Every k-mer inside a sequence must be new or continue a known path"""
    index, kmers, edges = {}, [], {}
    for si, item in enumerate([(ref, 1)] + [a if isinstance(a, tuple) else (a, 1) for a in alts]):
        seq, weight = item
        seq = seq.encode() if isinstance(seq, str) else bytes(seq)
        prev = None
        for i in range(len(seq) - k + 1):
            km = seq[i:i + k]
            if km not in index:
                index[km] = len(kmers)
                kmers.append(km)
            v = index[km]
            if prev is not None:
                e = edges.setdefault((prev, v), [si == 0, 0])
                e[1] += weight
            prev = v
    return graph(k, kmers, [(a, b, int(r), m, m) for (a, b), (r, m) in edges.items()], factor)


def cyclic(g):
    return P.StableGraph and P.has_cycles(R.Graph(g["k"], g["kmers"], g["edges"], g["vertex_absent"], g["edge_absent"]))


# ---- the shapes at which the kernel can go wrong ------------------------------------------------------------------------------------
def _dna(rng, n):
    return "".join(rng.choice("ACGT") for _ in range(n))


def _unique(rng, n, k):
    while True:
        s = _dna(rng, n)
        if len({s[i:i + k] for i in range(n - k + 1)}) == n - k + 1:
            return s


def _flip(c):
    return "ACGT"["ACGT".index(c) ^ 1]


def _snps(seq, every, last=False):
    """seq with a base flipped every `every` bases (fewer than k: no k-mer of it is a k-mer of the original), from the front or so
    that the last base is one of them"""
    start = (len(seq) - 1) % every if last else 0
    return "".join(_flip(c) if i % every == start else c for i, c in enumerate(seq))


def _count(g, kind):
    gr = R.Graph(g["k"], g["kmers"], g["edges"])
    return len(P.dangling_tails(gr) if kind == R.TAIL else P.dangling_heads(gr))


def tail_of(n_alt, n_ref, k=11):
    """one dangling tail whose alt path has n_alt vertices (the fork vertex included) over a reference path of n_ref: the tail
    follows the reference with a SNP every 10 bases, so it never meets it again, and runs on at random where the reference ends"""
    for seed in range(100):
        rng = random.Random(seed * 1000 + n_alt * 7 + n_ref)
        ref = _unique(rng, 30 + k + n_ref - 1, k)
        fork = len(ref) - (n_ref - 1)            # the fork vertex's k-mer ends in front of ref[fork]: n_ref - 1 reference vertices follow it
        tail = _snps((ref[fork:] + _dna(rng, n_alt))[:n_alt - 1], 10)
        g = threaded(k, ref, [ref[fork - k:fork] + tail])
        if len(g["kmers"]) == len(ref) - k + 1 + n_alt - 1 and _count(g, R.TAIL) == 1:
            return g


def head_of(n_alt, k=11):
    """one dangling head whose alt path has n_alt vertices (the reference vertex it runs into included)"""
    for seed in range(100):
        rng = random.Random(seed * 1000 + n_alt)
        ref = _unique(rng, 60 + n_alt + 2 * k, k)
        join = 40 + n_alt                         # the head's last own base lies in front of ref[join]
        own = _snps(ref[join - (n_alt - 1):join], 10, last=True)
        g = threaded(k, ref, [own + ref[join:join + k]])
        if len(g["kmers"]) == len(ref) - k + 1 + n_alt - 1 and _count(g, R.HEAD) == 1:
            return g


def many_tails(n, k=11):
    for seed in range(100):
        rng = random.Random(seed * 100 + n)
        ref = _unique(rng, 20 + 12 * n + 3 * k, k)
        reads = []
        for i in range(n):
            p = 15 + 12 * i + k
            reads.append(ref[p - k:p] + _flip(ref[p]) + ref[p + 1:p + 7])
        g = threaded(k, ref, reads)
        if _count(g, R.TAIL) == n and _count(g, R.HEAD) == 0:
            return g


def many_heads(n, k=11):
    for seed in range(100):
        rng = random.Random(seed * 100 + n)
        ref = _unique(rng, 30 + 14 * n + 3 * k, k)
        reads = []
        for i in range(n):
            p = 20 + 14 * i
            reads.append(ref[p:p + 3] + _flip(ref[p + 3]) + ref[p + 4:p + 8 + k])
        g = threaded(k, ref, reads)
        if _count(g, R.HEAD) == n and _count(g, R.TAIL) == 0:
            return g


def fork_below_a_non_reference_vertex(k=9):
    """a branch leaves the reference and forks into two tails: the fork vertex is no reference vertex, so each tail is the other's
    'reference path' (get_next_reference_vertex with allow_non_ref_paths).  The first tail, in NodeIndex order, merges into the
    second; the second then walks into the vertex that gained an in-edge and finds no path.  In the other order it is the second
    that merges"""
    rng = random.Random(23)
    ref = _unique(rng, 80, k)
    branch = ref[20:20 + k] + _flip(ref[20 + k]) + _dna(rng, 12)
    shared = _dna(rng, k - 2)                    # (shorter than a k-mer: the two tails never meet again)
    one = branch + "A" + shared
    two = branch + "C" + shared + _dna(rng, 2)
    return threaded(k, ref, [one, two])


def tail_below_the_reference_sink(k=9):
    """the first tail forks off the reference and merges back into it; the second hangs below the reference sink, and its walk up
    the reference stops at the vertex the first merged into -- in-degree 2, out-degree 1: no path.  Without that merge it would
    have walked on to the first tail's fork vertex"""
    rng = random.Random(29)
    ref = _unique(rng, 70, k)
    p = 30
    first = ref[p - k:p] + _flip(ref[p]) + ref[p + 1:p + 8]
    second = ref[-k:] + _dna(rng, 6)
    return threaded(k, ref, [first, second])


def random_regions(n=200, seed=41):
    """small random regions: k 3 to 15, references of 30 to 120 bases, a handful of reads with errors, CHAINS-pruned with factors
    0 to 2; cyclic graphs are dropped, as the caller drops them"""
    rng = random.Random(seed)
    out = []
    while len(out) < n:
        k, n_ref = rng.randrange(3, 16), rng.randrange(30, 121)
        ref = _dna(rng, n_ref)
        reads = []
        for _ in range(rng.randrange(1, 7)):
            a = rng.randrange(0, n_ref - k)
            b = min(n_ref, a + rng.randrange(k + 1, 60))
            s = list(ref[a:b])
            for _ in range(rng.randrange(0, 3)):
                i = rng.randrange(len(s))
                kind = rng.randrange(3)
                if kind == 0:
                    s[i] = _flip(s[i])
                elif kind == 1:
                    s.insert(i, rng.choice("ACGT"))
                else:
                    del s[i]
            if len(s) > k:
                reads.append("".join(s))
        g = from_region(ref, reads, k, rng.randrange(0, 3), chains=True)
        if g["kmers"] and not cyclic(g):
            out.append(g)
    return out


# ---- the golden cases as graphs ---------------------------------------------------------------------------------------------------
def tails_row(row):
    c = golden()
    ref_end, alt_end = row[0], row[1]
    return from_region(c["common_prefix"] + ref_end, [c["common_prefix"] + alt_end], c["tails"]["k"], c["tails"]["prune_factor"])


def heads_row(row):
    c = golden()
    return from_region(row[0], [row[1]], c["heads"]["k"], c["heads"]["prune_factor"])


def golden_graphs():
    """name -> (graph, Config)"""
    c = golden()
    out = {}
    for i, row in enumerate(c["tails"]["rows"]):
        out["tails_%02d" % i] = (tails_row(row), R.Config(ops=R.OP_TAILS, min_dangling_branch_length=c["tails"]["min_dangling_branch_length"], min_matching_bases=row[5]))
    for i, row in enumerate(c["heads"]["rows"]):
        out["heads_%02d" % i] = (heads_row(row), R.Config(ops=R.OP_HEADS, min_dangling_branch_length=c["heads"]["min_dangling_branch_length"], min_matching_bases=row[4]))
    for name in ("forked_with_suffix_code", "forked"):
        f = c[name]
        out[name] = (from_region(c["common_prefix"] + f["ref_end"], [c["common_prefix"] + r for r in f["reads_in_order"]], f["k"]),
                     R.Config(ops=R.OP_TAILS, min_dangling_branch_length=f["min_dangling_branch_length"], min_matching_bases=f["min_matching_bases"]))
    q = c["quirks"]["extension_refused_by_the_index_range"]
    out["quirk_extension_refused_by_the_index_range"] = (from_region(q["reference"], [q["alternate"]], q["k"], q["prune_factor"]),
                                                         R.Config(ops=R.OP_HEADS, min_dangling_branch_length=q["min_dangling_branch_length"], min_matching_bases=q["min_matching_bases"]))
    out["quirk_merge_index_past_the_reference_path"] = (tails_row(c["tails"]["rows"][12]), R.Config(ops=R.OP_TAILS, min_dangling_branch_length=4, min_matching_bases=0))
    for name, h in c["hand_graphs"].items():
        if "kmers" in h:
            for factor in h["expect_by_factor"]:
                out["hand_%s_factor_%s" % (name, factor)] = (graph(h["k"], [x.encode() for x in h["kmers"]], h["edges"], int(factor)),
                                                            R.Config(ops=h["ops"], min_dangling_branch_length=h["min_dangling_branch_length"]))
    for name, q in c["quirks"].items():
        if "ref_end" in q:
            g = from_region(c["common_prefix"] + q["ref_end"], [c["common_prefix"] + q["alt_end"]], q["k"], q["prune_factor"])
            out["quirk_" + name] = (g, R.Config(ops=R.OP_TAILS, min_dangling_branch_length=q["min_dangling_branch_length"], min_matching_bases=q["min_matching_bases"]))
    return out


# ---- a call: its arrays, and the restatement's answer in the call's layout ----------------------------------------------------------
def pack(graphs):
    """(regions, graph, masks, prune_factor, slots): the arguments of lorikeet_amd.assembly.recover_dangling_ends for these graphs in
    one call.  The layout is k-major: slot (k index, region r) holds graph r where its k is that k, and an empty graph elsewhere;
    slots[r] is graph r's slot"""
    ks = sorted({g["k"] for g in graphs})
    n = len(graphs)
    regions = [(b"".join(g["kmers"]), []) for g in graphs]
    vertex_off, edge_off, cols = [0], [0], {name: [] for name in ("vertex_seq", "vertex_pos", "edge_src", "edge_dst", "edge_is_ref", "edge_multiplicity",
                                                                  "edge_pruning_multiplicity", "vertex_absent", "edge_absent", "factor")}
    slots = [ks.index(g["k"]) * n + r for r, g in enumerate(graphs)]
    for ki, k in enumerate(ks):
        for g in graphs:
            mine = g["k"] == k
            nv, edges = (len(g["kmers"]), g["edges"]) if mine else (0, [])
            cols["vertex_seq"] += [0] * nv
            cols["vertex_pos"] += [v * k for v in range(nv)]
            for j, name in enumerate(("edge_src", "edge_dst", "edge_is_ref", "edge_multiplicity", "edge_pruning_multiplicity")):
                cols[name] += [e[j] for e in edges]
            cols["vertex_absent"] += (g["vertex_absent"] or [0] * nv) if mine else []
            cols["edge_absent"] += (g["edge_absent"] or [0] * len(edges)) if mine else []
            cols["factor"].append(g["factor"])
            vertex_off.append(vertex_off[-1] + nv)
            edge_off.append(edge_off[-1] + len(edges))
    arr = lambda name, dt: np.asarray(cols[name], dt)  # noqa: E731
    gd = dict(k=np.asarray(ks, np.uint32), vertex_off=np.asarray(vertex_off, np.uint32), edge_off=np.asarray(edge_off, np.uint32),
              vertex_seq=arr("vertex_seq", np.uint32), vertex_pos=arr("vertex_pos", np.uint32), edge_src=arr("edge_src", np.uint32),
              edge_dst=arr("edge_dst", np.uint32), edge_is_ref=arr("edge_is_ref", np.uint8), edge_multiplicity=arr("edge_multiplicity", np.uint32),
              edge_pruning_multiplicity=arr("edge_pruning_multiplicity", np.uint32))
    masks = dict(vertex_absent=arr("vertex_absent", np.uint8), edge_absent=arr("edge_absent", np.uint8))
    return regions, gd, masks, arr("factor", np.uint32), slots


_memo = {}


def one(g, cfg):
    key = (g["k"], tuple(g["kmers"]), tuple(g["edges"]), g["factor"], None if g["vertex_absent"] is None else (tuple(g["vertex_absent"]), tuple(g["edge_absent"])), cfg.key())
    if key not in _memo:
        _memo[key] = R.recover(g["k"], g["kmers"], g["edges"], g["factor"], cfg, g["vertex_absent"], g["edge_absent"])
    return _memo[key]


def expected(graphs, cfg):
    """the output arrays of the call pack(graphs) describes, from the restatement"""
    ks = sorted({g["k"] for g in graphs})
    k_max = max(ks) if ks else 0
    empty = dict(n_tails=0, n_tails_recovered=0, n_heads=0, n_heads_recovered=0, n_new_edges=0, n_new_vertices=0, end_vertex=[], end_kind=[],
                 end_status=[], end_alt_len=[], end_ref_len=[], end_n_cigar=[], end_cigar=[], end_edge=[], new_edge_src=[], new_edge_dst=[],
                 new_edge_multiplicity=[], new_edge_pruning_multiplicity=[], new_vertex_kmer=[], edge_removed=[])
    xs = [one(g, cfg) if g["k"] == k else empty for k in ks for g in graphs]
    o = {name: np.asarray([x[name] for x in xs], np.uint32) for name in PER_GRAPH}
    for off, count in zip(OFFSETS, (lambda x: len(x["end_vertex"]), lambda x: x["n_new_edges"], lambda x: x["n_new_vertices"])):
        o[off] = np.cumsum([0] + [count(x) for x in xs]).astype(np.uint32)
    for name in PER_END + PER_EDGE:
        o[name] = np.asarray([v for x in xs for v in x[name]], np.uint32)
    o["end_cigar"] = o["end_cigar"].reshape(-1, 4)
    o["new_vertex_kmer"] = np.asarray([list(km) + [0] * (k_max - len(km)) for x in xs for km in x["new_vertex_kmer"]], np.uint8).reshape(-1, k_max)
    o["edge_removed"] = np.asarray([v for x in xs for v in x["edge_removed"]], np.uint8)
    return o


def gpu_sets():
    """name -> (graphs, Config): every set the GPU file runs, each graph alone and all of a set in one call"""
    out = {}
    gg = golden_graphs()
    for name, (g, cfg) in gg.items():
        out.setdefault(("golden", cfg.key()), ([], cfg))[0].append(g)
    out = {"golden_%d" % i: v for i, (_, v) in enumerate(sorted(out.items(), key=lambda kv: str(kv[0])))}
    both = R.Config(min_dangling_branch_length=1)
    out["alt_paths"] = ([tail_of(n, 140) for n in (63, 64, 65, 129)] + [head_of(n) for n in (63, 64, 65, 129)], both)
    out["ref_paths"] = ([tail_of(6, n) for n in (64, 65, 130)], both)
    out["many_ends"] = ([many_tails(n) for n in (1, 64, 65)] + [many_heads(n) for n in (1, 64, 65)], both)
    out["conflicts"] = ([fork_below_a_non_reference_vertex(), tail_below_the_reference_sink()], R.Config(min_dangling_branch_length=2, min_matching_bases=1))
    return out


def census(sets):
    """how often the sets reach each end_status, an extension, and a graph in which a later end inspects a vertex whose edges an
    earlier end of the same kind changed (what makes n_rounds exceed 1 per kind)"""
    n = {name: 0 for name in R.STATUS_NAMES}
    n["extension"] = n["conflict"] = 0
    for graphs, cfg in sets:
        for g in graphs:
            x = one(g, cfg)
            for name in x["census"]:
                n[name] += 1
            n["conflict"] += conflicts(g, cfg, x)
    return n


def conflicts(g, cfg, x):
    """1 if some end's straight walk -- up single in-edges for a tail, down single out-edges for a head, on the graph recovery
    left -- arrives at an endpoint of an edge that an earlier end of the same kind added: a later end read what an earlier one
    changed"""
    gr, touched = x["graph"], {R.TAIL: set(), R.HEAD: set()}
    for v, kind, edge in zip(x["end_vertex"], x["end_kind"], x["end_edge"]):
        seen = set()
        while touched[kind] and v not in seen:
            if v in touched[kind]:
                return 1
            seen.add(v)
            nxt = gr.edges_directed(v, kind == R.HEAD)
            if len(nxt) != 1:
                break
            v = gr.edge_endpoints(nxt[0])[1 if kind == R.HEAD else 0]
        if edge != R.NONE:
            touched[kind].update((x["new_edge_src"][edge], x["new_edge_dst"][edge]))
    return 0
