"""A SERIAL restatement of the reference's k-best haplotype finder, beside the lines it restates -- what
phmm_assembly_best_paths (include/phmm.h) is held to.  F = src/graphs/k_best_haplotype_finder.rs,
G = src/graphs/graph_based_k_best_haplotype_finder.rs, K = src/graphs/k_best_haplotype.rs, P = src/graphs/path.rs.  Taken as
written, not repaired.  A graph is a dict: vertices (a list of bytes), edges (a list of (source, target, is_ref, multiplicity),
an edge's index its petgraph EdgeIndex), and either sources / sinks (lists: the reference's sets) or source / sink (one
index each, NONE for a missing end).  The depth-first walk is iterative; the queue is a literal binary heap driven by the
reference's cmp; log10 is math.log10, the C library's.  `census` names the quirks a graph reached."""
import math

NONE = 0xFFFFFFFF
OK, SKIPPED, NO_ENDS, NO_PATH, CYCLES_STAY, WEIGHT_RANGE, BUDGET = range(7)
MAX_WEIGHT = 1 << 20
EQUALS_REF = 0xFFFFFFFE
UNLIMITED = 0xFFFFFFFF   # usize::MAX
QUIRKS = ("cross or forward edge removed", "vertex removed", "cycles stay", "no path", "sink with out-edges", "K-th pop does not extend",
          "stops at K results", "tie by edge list", "tie by prefix", "tie of zero-edge paths", "NaN", "-inf", "source is a sink",
          "several sources", "budget", "weight range", "no ends", "vertex of 0 bytes", "cyclic", "queue above 64")


def log10(n):
    return math.log10(n) if n else -math.inf   # (0 as f64).log10()


def ends(g):
    if "sources" in g:
        return sorted(set(g["sources"])), set(g["sinks"])
    return [g["source"]], {g["sink"]}


def out_edges(g, gone):
    """petgraph: the out-edges of a vertex iterate newest first"""
    out = [[] for _ in g["vertices"]]
    for e in range(len(g["edges"]) - 1, -1, -1):
        if not gone[e]:
            out[g["edges"][e][0]].append(e)
    return out


def is_cyclic(g):
    """is_cyclic_directed over the whole graph (F:78), parts no source reaches included"""
    n = len(g["vertices"])
    indeg = [0] * n
    for s, d, _, _ in g["edges"]:
        indeg[d] += 1
    todo, peeled = [v for v in range(n) if not indeg[v]], 0
    out = out_edges(g, [0] * len(g["edges"]))
    while todo:
        v = todo.pop()
        peeled += 1
        for e in out[v]:
            d = g["edges"][e][1]
            indeg[d] -= 1
            if not indeg[d]:
                todo.append(d)
    return peeled < n


def remove_cycles(g, census):
    """F:87-182.  Returns (found_some_path, edges_to_remove, vertices_to_remove)."""
    sources, sinks = ends(g)
    out = out_edges(g, [0] * len(g["edges"]))
    edges_to_remove, vertices_to_remove, found = set(), set(), False
    for source in sources:                       # F:95 (the sets are shared, the walks independent: any order)
        parent_vertices = set()                  # F:96, a fresh one per source; never shrunk on return
        if source in sinks:                      # F:143
            found = True
            continue
        parent_vertices.add(source)              # F:157
        stack = [[source, 0, False]]             # vertex, next out-edge, reaches_sink
        while stack:
            top = stack[-1]
            v, at = top[0], top[1]
            if at < len(out[v]):
                top[1] += 1
                e = out[v][at]
                child = g["edges"][e][1]
                if child in parent_vertices:     # F:163: ANY visited vertex, not only an ancestor
                    edges_to_remove.add(e)
                    census.add("cross or forward edge removed")   # (or a back edge: the hand case pins the cross edge)
                elif child in sinks:             # F:143 in the child's call: true at once, unmarked, unexplored
                    top[2] = True
                else:
                    parent_vertices.add(child)
                    stack.append([child, 0, False])
            else:
                stack.pop()
                if not top[2]:                   # F:177
                    vertices_to_remove.add(v)
                    census.add("vertex removed")
                if stack:
                    stack[-1][2] = stack[-1][2] or top[2]   # F:173
                else:
                    found = found or top[2]      # F:97-103
    return found, edges_to_remove, vertices_to_remove


class Candidate:
    """KBestHaplotype: score, is_reference, the path's edges and last vertex"""
    __slots__ = ("score", "is_ref", "edges", "first", "last")

    def __init__(self, score, is_ref, edges, first, last):
        self.score, self.is_ref, self.edges, self.first, self.last = score, is_ref, edges, first, last


def ordered_float_cmp(a, b):
    """OrderedFloat::cmp: NaN is greatest and equal to itself; -0.0 == 0.0"""
    if a != a or b != b:
        return (a != a) - (b != b)
    return (a > b) - (a < b)


def cmp(a, b, census=None):
    """K:103-112: by score, then other.edges.cmp(self.edges) -- the smaller list is the greater path, a proper prefix before its
    extension.  Zero-edge paths of several sources tie completely in the reference; the contract takes the lower vertex first."""
    c = ordered_float_cmp(a.score, b.score)
    if c:
        return c
    if a.edges != b.edges:
        if census is not None:
            n = min(len(a.edges), len(b.edges))
            census.add("tie by prefix" if a.edges[:n] == b.edges[:n] else "tie by edge list")
        return (b.edges > a.edges) - (b.edges < a.edges)
    if census is not None:
        census.add("tie of zero-edge paths")
    return (b.first > a.first) - (b.first < a.first)


class BinaryHeap:
    """std::collections::BinaryHeap as a literal array heap: push sifts up, pop moves the last element to the root and sifts down"""

    def __init__(self, census):
        self.data, self.census = [], census

    def push(self, x):
        d = self.data
        d.append(x)
        i = len(d) - 1
        while i and cmp(d[i], d[(i - 1) // 2], self.census) > 0:
            d[i], d[(i - 1) // 2] = d[(i - 1) // 2], d[i]
            i = (i - 1) // 2

    def pop(self):
        d = self.data
        top, last = d[0], d.pop()
        if d:
            d[0], i = last, 0
            while True:
                c = 2 * i + 1
                if c >= len(d):
                    break
                if c + 1 < len(d) and cmp(d[c + 1], d[c], self.census) > 0:
                    c += 1
                if cmp(d[c], d[i], self.census) <= 0:
                    break
                d[i], d[c] = d[c], d[i]
                i = c
        return top

    def __len__(self):
        return len(self.data)


class TakeTheMaximum:
    """the same queue as a plain list: pop is the maximum under cmp -- what a heap of elements no two of which compare equal returns"""

    def __init__(self, census):
        self.data, self.census = [], census

    def push(self, x):
        self.data.append(x)

    def pop(self):
        best = 0
        for i in range(1, len(self.data)):
            if cmp(self.data[i], self.data[best], self.census) > 0:
                best = i
        return self.data.pop(best)

    def __len__(self):
        return len(self.data)


def best_paths(g, max_paths=128, max_nodes=1 << 16, status=OK, heap=True):
    """One graph.  Returns a dict: status, paths (score, is_ref, edges, bases in pop order), n_popped, edge_removed and
    vertex_removed (a byte per input element), census."""
    nv, ne = len(g["vertices"]), len(g["edges"])
    census = set()
    res = dict(status=OK, paths=[], n_popped=0, edge_removed=[0] * ne, vertex_removed=[0] * nv, census=census)
    if status != OK:
        res["status"] = SKIPPED
        return res
    if "sources" not in g and NONE in (g["source"], g["sink"]):   # A:739-742
        res["status"] = NO_ENDS
        census.add("no ends")
        return res
    totals = [0] * nv
    for s, _, _, m in g["edges"]:
        totals[s] += m
    if nv and max(totals) > MAX_WEIGHT:
        res["status"] = WEIGHT_RANGE
        census.add("weight range")
        return res
    sources, sinks = ends(g)
    if any(not len(v) for v in g["vertices"]):
        census.add("vertex of 0 bytes")
    if len(sources) > 1:
        census.add("several sources")
    if set(sources) & sinks:
        census.add("source is a sink")
    gone_v = [0] * nv
    gone_e = [0] * ne
    if is_cyclic(g):                              # F:78
        census.add("cyclic")
        found, edges_to_remove, vertices_to_remove = remove_cycles(g, census)
        if not found:                             # F:106
            res["status"] = NO_PATH
            census.add("no path")
            return res
        if not edges_to_remove and not vertices_to_remove:   # F:110
            res["status"] = CYCLES_STAY
            census.add("cycles stay")
            return res
        for v in vertices_to_remove:
            gone_v[v] = 1
        for e, (s, d, _, _) in enumerate(g["edges"]):   # F:117-118: remove_all_vertices takes the vertices' edges along
            gone_e[e] = (1 if e in edges_to_remove else 0) | (2 if gone_v[s] or gone_v[d] else 0)
        res["edge_removed"], res["vertex_removed"] = gone_e, gone_v
    out = out_edges(g, gone_e)
    # G:64-132
    queue = (BinaryHeap if heap else TakeTheMaximum)(census)
    created = 0
    for s in sources:                             # G:75-80
        created += 1
        if created > max_nodes:
            res["status"] = BUDGET
            census.add("budget")
            return res
        queue.push(Candidate(0.0, True, (), s, s))   # K:28-38
    counts = [0] * nv                             # G:83-87: the vertices of the graph behind the removal
    results = []
    while len(queue) and len(results) < max_paths:   # G:94 (UNLIMITED is usize::MAX)
        if len(queue) > 64:
            census.add("queue above 64")
        p = queue.pop()
        res["n_popped"] += 1
        v = p.last
        if v in sinks:                            # G:98-103: a result; not extended, out-edges or not
            results.append(p)
            if out[v]:
                census.add("sink with out-edges")
        elif not gone_v[v]:                       # G:104
            counts[v] += 1
            if counts[v] < max_paths:             # G:108
                total = sum(g["edges"][e][3] for e in out[v])   # G:112-116, usize
                for e in out[v]:                  # G:118-124
                    _, d, is_ref, m = g["edges"][e]
                    created += 1
                    if created > max_nodes:
                        res.update(status=BUDGET, n_popped=res["n_popped"])
                        census.add("budget")
                        return res
                    score = p.score + (log10(m) - log10(total))   # K:49-53 with K:86-91: three roundings
                    if score != score:
                        score = math.nan          # one NaN: 0x7ff8000000000000, whatever sign the subtraction gave
                        census.add("NaN")
                    elif score == -math.inf:
                        census.add("-inf")
                    queue.push(Candidate(score, p.is_ref and bool(is_ref), p.edges + (e,), p.first, d))
            elif out[v]:
                census.add("K-th pop does not extend")
    res["n_created"] = created                   # the search tree's nodes, the sources' included: what the budget bounds
    if len(results) == max_paths and len(queue):
        census.add("stops at K results")
    for p in results:
        bases = g["vertices"][p.first] + b"".join(g["vertices"][g["edges"][e][1]] for e in p.edges)   # P:234-267
        res["paths"].append(dict(score=p.score, is_ref=p.is_ref, edges=list(p.edges), bases=bases))
    return res


def first_equal(regions, n_k, per_graph_paths):
    """A:770 with Haplotype::eq on bytes.  regions: the reference bytes per region; per_graph_paths: for each graph (k-major) its
    paths' bytes in rank order.  Returns a list over all paths of the call: NONE, EQUALS_REF or the earliest equal path."""
    n_regions = len(regions)
    starts, n = [], 0
    for paths in per_graph_paths:
        starts.append(n)
        n += len(paths)
    answer = [NONE] * n
    for r in range(n_regions):
        seen = {}
        for k in range(n_k):
            g = k * n_regions + r
            for rank, bases in enumerate(per_graph_paths[g]):
                p = starts[g] + rank
                if bases == regions[r]:
                    answer[p] = EQUALS_REF
                elif bases in seen:
                    answer[p] = seen[bases]
                else:
                    seen[bases] = p
    return answer
