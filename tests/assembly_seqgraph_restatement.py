"""A SERIAL restatement of what the reference's assembler does between the pruned read-threading graph and simplify_graph,
statement by statement beside the reference's lines: B = src/graphs/base_graph.rs, S = src/graphs/seq_graph.rs, A =
src/read_threading/read_threading_assembler.rs.  The steps are to_sequence_graph (B:54-84), clean_non_ref_paths (B:716-768), the
first zip_linear_chains (S:189-369, called at A:1251), remove_singleton_orphan_vertices (B:392-406) and
remove_vertices_not_connected_to_ref_regardless_of_edge_direction (B:774-793 with B:686-709).  It walks the StableGraph model of
assembly_prune_restatement.py -- indices stay when an element goes, edges_directed runs from the newest edge to the oldest --
with the reference's heaps and its chain walk, and shares nothing with the order-free statement phmm_assembly_seqgraph computes
on the device.

Numbering: petgraph's reuse of vacant slots is not modelled.  A new vertex or edge takes a fresh index behind all existing
ones, and the result is the present elements in ascending model index, renumbered compactly."""
import heapq

OK, SKIPPED, REFERENCE_FAILS = 0, 1, 2
HAS_CYCLE, NO_REF_ENDS = 1, 2
NONE = 0xFFFFFFFF


class ReferenceFails(Exception):
    """the reference would panic here"""


class SeqGraph:
    """petgraph's StableGraph with vertex bytes and edge weights; add_node / add_edge take a fresh index"""

    def __init__(self):
        self.node, self.seq, self.members = [], [], []   # members: the input vertices whose bytes the vertex holds
        self.edge, self.is_ref, self.multiplicity = [], [], []
        self.outgoing, self.incoming = [], []
        self.count = 0

    def add_node(self, seq, members):
        self.node.append(True)
        self.seq.append(bytes(seq))
        self.members.append(list(members))
        self.outgoing.append([])
        self.incoming.append([])
        self.count += 1
        return len(self.node) - 1

    def add_edge(self, a, b, is_ref, multiplicity):
        assert self.node[a] and self.node[b]
        self.edge.append((a, b))
        self.is_ref.append(bool(is_ref))
        self.multiplicity.append(int(multiplicity))
        e = len(self.edge) - 1
        self.outgoing[a].append(e)
        self.incoming[b].append(e)
        return e

    def node_indices(self):
        return [v for v, there in enumerate(self.node) if there]

    def edges_directed(self, v, out):
        return list(reversed(self.outgoing[v] if out else self.incoming[v]))

    def remove_edge(self, e):
        a, b = self.edge[e]
        self.outgoing[a].remove(e)
        self.incoming[b].remove(e)
        self.edge[e] = None

    def remove_node(self, v):
        for e in self.edges_directed(v, True) + [e for e in self.edges_directed(v, False) if self.edge[e][0] != v]:
            self.remove_edge(e)
        self.node[v] = False
        self.count -= 1


def in_degree_of(g, v):                                                    # B:168-172
    return len(g.incoming[v])


def out_degree_of(g, v):                                                   # B:178-182
    return len(g.outgoing[v])


def is_ref_source(g, v):                                                   # B:339-360
    if any(g.is_ref[e] for e in g.edges_directed(v, False)):
        return False
    if any(g.is_ref[e] for e in g.edges_directed(v, True)):
        return True
    return g.count == 1                                                    # B:359


def is_ref_sink(g, v):                                                     # B:366-387
    if any(g.is_ref[e] for e in g.edges_directed(v, True)):
        return False
    if any(g.is_ref[e] for e in g.edges_directed(v, False)):
        return True
    return g.count == 1                                                    # B:386


def is_reference_node(g, v):                                               # B:130-146
    if any(g.is_ref[e] for e in g.edges_directed(v, False)) or any(g.is_ref[e] for e in g.edges_directed(v, True)):
        return True
    return g.count == 1                                                    # B:144: vertices are told apart by an identity code


def get_reference_source_vertex(g):                                        # B:411-417
    return next((v for v in g.node_indices() if is_ref_source(g, v)), None)


def get_reference_sink_vertex(g):                                          # B:422-428
    return next((v for v in g.node_indices() if is_ref_sink(g, v)), None)


def remove_singleton_orphan_vertices(g):                                   # B:392-406
    to_remove = [v for v in g.node_indices()
                 if in_degree_of(g, v) == 0 and out_degree_of(g, v) == 0 and not is_ref_source(g, v)]   # listed before any goes
    for v in to_remove:
        g.remove_node(v)
    return to_remove


def to_sequence_graph(n_vertices, edges, kmers, vertex_absent, edge_absent):   # B:54-84
    """kmers[v]: the k bytes of input vertex v.  Returns the graph and, per input vertex, its sequence vertex or None."""
    present_e = [e for e in range(len(edges)) if not (edge_absent is not None and edge_absent[e])]
    has_in = set(edges[e][1] for e in present_e)
    g, vertex_map = SeqGraph(), [None] * n_vertices
    for dv in range(n_vertices):                                           # B:59-69
        if vertex_absent is not None and vertex_absent[dv]:
            continue
        kmer = bytes(kmers[dv])
        vertex_map[dv] = g.add_node(kmer if dv not in has_in else kmer[-1:], [dv])   # get_additional_sequence(is_source)
    for e in present_e:                                                    # B:72-81
        a, b, is_ref, multiplicity = edges[e]
        g.add_edge(vertex_map[a], vertex_map[b], is_ref, multiplicity)
    return g, vertex_map


def clean_non_ref_paths(g, census):                                        # B:716-768
    """Returns the number of edges removed.  The reference pops an edge index it has removed already -- and panics on its
    weight -- when a vertex's edge list is pushed a second time and still holds a non-reference edge; whether the edge is
    still there at the second push depends on the heap's order.  phmm_assembly_seqgraph's contract is the order-free
    superset: a list that held a non-reference edge and is pushed twice fails the graph."""
    if get_reference_source_vertex(g) is None or get_reference_sink_vertex(g) is None:   # B:717-720
        census.add("clean: an end is missing")
        return 0
    removed = 0
    for out, what in ((False, "in front of the source"), (True, "behind the sink")):
        end = get_reference_sink_vertex(g) if out else get_reference_source_vertex(g)    # B:727, B:748: looked up again
        if end is None:
            raise ReferenceFails("the sink is gone")                       # B:748 unwrap
        held_non_ref = {v: any(not g.is_ref[e] for e in g.edges_directed(v, out)) for v in g.node_indices()}
        pushes = {}
        edges_to_check = []                                                # B:723: a BinaryHeap, the largest index first

        def push(v):
            pushes[v] = pushes.get(v, 0) + 1
            for e in g.edges_directed(v, out):                             # B:724-731, 736-740
                heapq.heappush(edges_to_check, -e)

        push(end)
        panics = False
        while edges_to_check:                                              # B:733, B:754
            e = -heapq.heappop(edges_to_check)                             # B:734
            if g.edge[e] is None:                                          # B:735 edge_weight(e).unwrap()
                panics = True
                continue
            if not g.is_ref[e]:                                            # B:735
                push(g.edge[e][1 if out else 0])                           # B:736-740
                g.remove_edge(e)                                           # B:741
                removed += 1
                census.add("clean removes " + what)
        fails = any(n >= 2 and held_non_ref[v] for v, n in pushes.items())
        assert not panics or fails
        if fails:
            census.add("reference fails " + what + (": it panics in this order" if panics else ": it survives in this order"))
            raise ReferenceFails("a list with a non-reference edge is pushed twice")
    if remove_singleton_orphan_vertices(g):                                # B:766
        census.add("clean orphans a vertex")
    return removed


def is_linear_chain_start(g, source):                                      # S:227-238
    if out_degree_of(g, source) != 1:
        return False
    if in_degree_of(g, source) != 1:
        return True
    return out_degree_of(g, g.edge[g.edges_directed(source, False)[0]][0]) > 1


def trace_linear_chain(g, zip_start, census):                              # S:250-294
    linear_chain = [zip_start]
    last_is_ref = is_reference_node(g, zip_start)                          # S:253
    last = zip_start
    while True:
        if out_degree_of(g, last) != 1:                                    # S:257
            break
        target = g.edge[g.edges_directed(last, True)[0]][1]                # S:263-273
        if in_degree_of(g, target) != 1 or last == target:                 # S:275
            break
        target_is_ref = is_reference_node(g, target)                       # S:280
        if last_is_ref != target_is_ref:                                   # S:281
            census.add("zip: a reference break")
            break
        linear_chain.append(target)                                        # S:286
        last, last_is_ref = target, target_is_ref                          # S:289-290
    return linear_chain


def merge_linear_chain_vertex(g, linear_chain, census):                    # S:311-352
    first, last = linear_chain[0], linear_chain[-1]
    if first == last:                                                      # S:321
        return None
    added = g.add_node(b"".join(g.seq[v] for v in linear_chain), [dv for v in linear_chain for dv in g.members[v]])   # S:327-329, S:354-369
    for e in g.edges_directed(last, True):                                 # S:332-338
        if g.edge[e][1] == first:
            census.add("zip: last -> first")
        if len(g.members[g.edge[e][1]]) > 1:
            census.add("zip: chain into chain, the target merged first")
        g.add_edge(added, g.edge[e][1], g.is_ref[e], g.multiplicity[e])
    for e in g.edges_directed(first, False):                               # S:339-345: the list as it stands now
        if len(g.members[g.edge[e][0]]) > 1 and g.edge[e][0] != added:
            census.add("zip: chain into chain, the source merged first")
        g.add_edge(g.edge[e][0], added, g.is_ref[e], g.multiplicity[e])
    for v in linear_chain:                                                 # S:347-349
        g.remove_node(v)
    return added


def zip_linear_chains(g, census):                                          # S:189-214
    zip_starts = [v for v in g.node_indices() if is_linear_chain_start(g, v)]   # S:191-196
    merged = 0
    for zip_start in zip_starts:                                           # S:206-211
        if merge_linear_chain_vertex(g, trace_linear_chain(g, zip_start, census), census) is not None:
            merged += 1
    if any(in_degree_of(g, v) == 1 and out_degree_of(g, v) == 1 and len(g.members[v]) == 1 and g.edge[g.incoming[v][0]][0] != v and
           out_degree_of(g, g.edge[g.incoming[v][0]][0]) == 1 and in_degree_of(g, g.edge[g.outgoing[v][0]][1]) == 1 for v in g.node_indices()):
        census.add("zip: an interior vertex stays (a ring, or behind a reference break)")
    return merged


def get_all_connected_nodes_from_node(g, starting_node, out):             # B:686-709
    to_visit, visited = [-starting_node], set()
    while to_visit:
        v = -heapq.heappop(to_visit)
        if v not in visited:
            visited.add(v)
            for e in g.edges_directed(v, out):
                heapq.heappush(to_visit, -g.edge[e][1 if out else 0])
    return visited


def remove_vertices_not_connected_to_ref_regardless_of_edge_direction(g, census):   # B:774-793
    to_remove = set(g.node_indices())                                      # B:775
    ref_v = get_reference_source_vertex(g)                                 # B:777
    if ref_v is None:
        census.add("connectivity: no reference source")
    else:
        to_remove -= get_all_connected_nodes_from_node(g, ref_v, False)    # B:781-783
        to_remove -= get_all_connected_nodes_from_node(g, ref_v, True)     # B:785-787
        to_remove.discard(ref_v)                                           # B:788
        # (a vertex that is weakly connected to the source and goes all the same)
        weak, grew = {ref_v}, True
        while grew:
            grew = False
            for e in g.edge:
                if e is not None and (e[0] in weak) != (e[1] in weak):
                    weak.update(e)
                    grew = True
        if to_remove & weak:
            census.add("connectivity: a weakly connected vertex goes")
    for v in sorted(to_remove):                                            # B:779, B:790
        g.remove_node(v)
    return len(to_remove)


def empty(status, n_vertices):
    return dict(seq_status=status, n_seq_vertices=0, n_seq_edges=0, n_seq_bases=0, n_chains_zipped=0, n_removed_clean=0,
                n_removed_unconnected=0, seq_ref_source=NONE, seq_ref_sink=NONE, seq_vertex_base_off=[], seq_vertex_first=[],
                seq_vertex_n_merged=[], seq_edge_src=[], seq_edge_dst=[], seq_edge_is_ref=[], seq_edge_multiplicity=[], seq_bases=b"",
                vertex_to_seq=[NONE] * n_vertices, census=set())


def sequence_graph(n_vertices, edges, kmers, vertex_absent=None, edge_absent=None, graph_flags=0):
    """One graph as phmm_assembly_seqgraph reports it.  edges: [(source, target, is_ref, multiplicity)] in EdgeIndex order;
    kmers[v]: the k bytes of vertex v (anything for an absent one)."""
    if graph_flags & (HAS_CYCLE | NO_REF_ENDS):
        res = empty(SKIPPED, n_vertices)
        res["census"].add("skipped")
        return res
    census = set()
    g, _ = to_sequence_graph(n_vertices, edges, kmers, vertex_absent, edge_absent)             # A:1154
    if g.count == 1:
        census.add("one node")
    if any(len(s) > 1 for s in g.seq):
        census.add("a source vertex carries k bytes")
    try:
        n_removed_clean = clean_non_ref_paths(g, census)                   # A:1244 (B:716)
    except ReferenceFails:
        res = empty(REFERENCE_FAILS, n_vertices)
        res["census"] = census
        return res
    n_chains_zipped = zip_linear_chains(g, census)                         # A:1251
    if remove_singleton_orphan_vertices(g):                                # A:1258
        census.add("an orphan behind the zip")
    n_removed_unconnected = remove_vertices_not_connected_to_ref_regardless_of_edge_direction(g, census)   # A:1259
    # ---- the present elements in ascending model index, renumbered compactly ---------------------------------------------------
    new_v = {v: i for i, v in enumerate(g.node_indices())}
    live_e = [e for e in range(len(g.edge)) if g.edge[e] is not None]
    source, sink = get_reference_source_vertex(g), get_reference_sink_vertex(g)
    base_off, at = [], 0
    for v in g.node_indices():
        base_off.append(at)
        at += len(g.seq[v])
    vertex_to_seq = [NONE] * n_vertices                                    # an input vertex maps to the vertex that holds its bytes
    for v in g.node_indices():
        for dv in g.members[v]:
            vertex_to_seq[dv] = new_v[v]
    return dict(seq_status=OK, n_seq_vertices=len(new_v), n_seq_edges=len(live_e), n_seq_bases=at, n_chains_zipped=n_chains_zipped,
                n_removed_clean=n_removed_clean, n_removed_unconnected=n_removed_unconnected,
                seq_ref_source=NONE if source is None else new_v[source], seq_ref_sink=NONE if sink is None else new_v[sink],
                seq_vertex_base_off=base_off, seq_vertex_first=[g.members[v][0] for v in g.node_indices()],
                seq_vertex_n_merged=[len(g.members[v]) for v in g.node_indices()],
                seq_edge_src=[new_v[g.edge[e][0]] for e in live_e], seq_edge_dst=[new_v[g.edge[e][1]] for e in live_e],
                seq_edge_is_ref=[int(g.is_ref[e]) for e in live_e], seq_edge_multiplicity=[g.multiplicity[e] for e in live_e],
                seq_bases=b"".join(g.seq[v] for v in g.node_indices()), vertex_to_seq=vertex_to_seq, census=census)
