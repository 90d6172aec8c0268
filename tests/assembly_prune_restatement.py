"""A SERIAL restatement of what the reference's assembler does to the raw read-threading graph before it looks for paths,
statement by statement beside the reference's lines: C = src/graphs/chain_pruner.rs, L = src/graphs/low_weight_chain_pruner.rs,
B = src/graphs/base_graph.rs, R = src/read_threading/read_threading_graph.rs, A = src/read_threading/read_threading_assembler.rs.
It walks a small model of petgraph's StableGraph -- vacant slots, edges_directed newest first -- with the reference's deque,
its DFS and its heaps, and shares nothing with the order-free statement phmm_assembly_prune computes on the device (DESIGN.md
(s)): no interior vertices, no chain heads, no peeling."""
import heapq
from collections import deque

OP_CHAINS, OP_CONNECT = 1, 2
HAS_CYCLE, NO_REF_ENDS = 1, 2
ABSENT, REMOVED_CHAINS, REMOVED_CONNECT, DANGLING_TAIL, DANGLING_HEAD = 1, 2, 4, 8, 16
NONE = 0xFFFFFFFF


class StableGraph:
    """petgraph::stable_graph::StableGraph as the reference uses it: indices stay when an element goes; edges_directed walks a
    vertex's edges from the newest to the oldest"""

    def __init__(self, n_vertices, edges, vertex_absent=None, edge_absent=None):
        self.node = [not (vertex_absent is not None and vertex_absent[v]) for v in range(n_vertices)]
        self.count = sum(self.node)               # node_indices().count()
        self.edge = [None] * len(edges)           # (source, target) or None = vacant
        self.is_ref = [bool(e[2]) for e in edges]
        self.pruning_multiplicity = [int(e[3]) for e in edges]
        self.outgoing = [[] for _ in range(n_vertices)]
        self.incoming = [[] for _ in range(n_vertices)]
        for e, (a, b, _, _) in enumerate(edges):
            if edge_absent is not None and edge_absent[e]:
                continue
            assert self.node[a] and self.node[b]
            self.edge[e] = (a, b)
            self.outgoing[a].append(e)
            self.incoming[b].append(e)

    def node_indices(self):
        return [v for v, there in enumerate(self.node) if there]

    def edges_directed(self, v, out):
        return list(reversed(self.outgoing[v] if out else self.incoming[v]))

    def edge_endpoints(self, e):
        return self.edge[e]

    def remove_edge(self, e):
        if self.edge[e] is None:
            return False
        a, b = self.edge[e]
        self.outgoing[a].remove(e)
        self.incoming[b].remove(e)
        self.edge[e] = None
        return True

    def remove_node(self, v):
        """with its edges, as petgraph does; returns them"""
        gone = self.edges_directed(v, True) + [e for e in self.edges_directed(v, False) if self.edge[e][0] != v]
        for e in gone:
            self.remove_edge(e)
        self.node[v] = False
        self.count -= 1
        return gone

    def externals(self, out):
        """vertices without an edge in that direction (Direction::Incoming = the sources)"""
        return [v for v in self.node_indices() if not (self.outgoing[v] if out else self.incoming[v])]


def in_degree_of(g, v):                                                    # B:168-172
    return len(g.edges_directed(v, False))


def out_degree_of(g, v):                                                   # B:178-182
    return len(g.edges_directed(v, True))


def find_chain(g, start_edge, census):                                     # C:86-118
    edges = [start_edge]                                                   # C:90
    first_vertex_id, last_vertex_id = g.edge_endpoints(start_edge)         # C:91-93
    while True:
        out_edges = set(g.edges_directed(last_vertex_id, True))            # C:101-105
        if len(out_edges) != 1 or in_degree_of(g, last_vertex_id) > 1 or last_vertex_id == first_vertex_id:   # C:106-109
            census.add("chain ends: no out-edge" if not out_edges else "chain ends: several out-edges" if len(out_edges) > 1
                       else "chain ends: several in-edges" if in_degree_of(g, last_vertex_id) > 1 else "chain ends: back at its start")
            break
        next_edge = next(iter(out_edges))                                  # C:112
        edges.append(next_edge)                                            # C:113
        last_vertex_id = g.edge_endpoints(next_edge)[1]                    # C:114
    return last_vertex_id, edges                                           # C:117


def find_all_chains(g, census):                                            # C:58-80
    chain_starts = deque(g.externals(False))                               # C:61
    chains = deque()
    already_seen = set(chain_starts)                                       # C:63-66
    while chain_starts:                                                    # C:67
        chain_start = chain_starts.popleft()                               # C:68
        for out_edge in g.edges_directed(chain_start, True):               # C:69
            chain = find_chain(g, out_edge, census)                        # C:70
            chain_end = chain[0]                                           # C:71
            chains.append(chain)                                           # C:72
            if chain_end not in already_seen:                              # C:73
                chain_starts.append(chain_end)                             # C:74
                already_seen.add(chain_end)                                # C:75
            else:
                census.add("chain end seen before")
    return chains


def needs_pruning(g, chain, prune_factor):                                 # L:24-36
    return all(g.pruning_multiplicity[e] < prune_factor and not g.is_ref[e] for e in chain[1])   # L:34


def is_ref_source(g, v):                                                   # B:339-360
    if any(g.is_ref[e] for e in g.edges_directed(v, False)):               # B:341-347
        return False
    if any(g.is_ref[e] for e in g.edges_directed(v, True)):                # B:350-356
        return True
    return g.count == 1                                                    # B:359


def is_ref_sink(g, v):                                                     # B:366-387
    if any(g.is_ref[e] for e in g.edges_directed(v, True)):                # B:368-374
        return False
    if any(g.is_ref[e] for e in g.edges_directed(v, False)):               # B:377-383
        return True
    return g.count == 1                                                    # B:386


def is_singleton_orphan(g, v):                                             # B:404-406
    return in_degree_of(g, v) == 0 and out_degree_of(g, v) == 0 and not is_ref_source(g, v)


def remove_singleton_orphan_vertices(g):                                   # B:392-402
    to_remove = [v for v in g.node_indices() if is_singleton_orphan(g, v)]  # B:395-399: listed before any goes
    for v in to_remove:                                                    # B:401, B:314-321
        g.remove_node(v)
    return to_remove


def prune_low_weight_chains(g, prune_factor, census):                      # C:39-56
    chains = find_all_chains(g, census)                                    # C:46
    chains_to_remove = [chain for chain in chains if needs_pruning(g, chain, prune_factor)]   # C:49, C:182-185
    removed_edges = []
    for chain in chains_to_remove:                                         # C:51-53
        for e in chain[1]:                                                 # B:326-333
            if g.remove_edge(e):
                removed_edges.append(e)
    orphans = remove_singleton_orphan_vertices(g)                          # C:55
    return chains, chains_to_remove, removed_edges, orphans


def get_reference_source_vertex(g):                                        # B:411-417
    return next((v for v in g.node_indices() if is_ref_source(g, v)), None)


def get_reference_sink_vertex(g):                                          # B:422-428
    return next((v for v in g.node_indices() if is_ref_sink(g, v)), None)


def has_cycles(g):                                                         # B:615-617: petgraph::algo::is_cyclic_directed, a DFS
    WHITE, GREY, BLACK = 0, 1, 2                                           # that meets a vertex still on its stack
    colour = {v: WHITE for v in g.node_indices()}
    for root in g.node_indices():
        if colour[root] != WHITE:
            continue
        colour[root] = GREY
        stack = [(root, iter(g.edges_directed(root, True)))]
        while stack:
            v, it = stack[-1]
            e = next(it, None)
            if e is None:
                colour[v] = BLACK
                stack.pop()
                continue
            w = g.edge_endpoints(e)[1]
            if colour[w] == GREY:
                return True
            if colour[w] == WHITE:
                colour[w] = GREY
                stack.append((w, iter(g.edges_directed(w, True))))
    return False


def dangling_tails(g):                                                     # R:792-797
    return [v for v in g.node_indices() if out_degree_of(g, v) == 0 and not is_ref_sink(g, v)]


def dangling_heads(g):                                                     # R:837-842
    return [v for v in g.node_indices() if in_degree_of(g, v) == 0 and not is_ref_source(g, v)]


def get_all_connected_nodes_from_node(g, starting_node, out):             # B:686-709
    to_visit = [-starting_node]                                            # B:691-693: a BinaryHeap, the largest index first
    visited = set()
    while to_visit:                                                        # B:696
        v = -heapq.heappop(to_visit)                                       # B:697
        if v not in visited:                                               # B:698
            visited.add(v)                                                 # B:699
            for e in g.edges_directed(v, out):                             # B:700-704: neighbors_directed
                heapq.heappush(to_visit, -g.edge_endpoints(e)[1 if out else 0])
    return visited


def remove_paths_not_connected_to_ref(g):                                  # B:626-656
    source, sink = get_reference_source_vertex(g), get_reference_sink_vertex(g)
    assert source is not None and sink is not None                         # B:627-631 panics
    on_path_from_ref_source = get_all_connected_nodes_from_node(g, source, True)    # B:634-637
    on_path_from_ref_sink = get_all_connected_nodes_from_node(g, sink, False)       # B:640-643
    vertices_to_remove = set(g.node_indices())                             # B:646
    on_path_from_ref_source = {v for v in on_path_from_ref_source if v in on_path_from_ref_sink}   # B:647
    vertices_to_remove = sorted(v for v in vertices_to_remove if v not in on_path_from_ref_source)  # B:648
    removed_edges = []
    for v in vertices_to_remove:                                           # B:655
        removed_edges += g.remove_node(v)
    return vertices_to_remove, removed_edges


def prune(n_vertices, edges, prune_factor, ops, vertex_absent=None, edge_absent=None):
    """One graph as phmm_assembly_prune reports it.  edges: [(source, target, is_ref, pruning multiplicity)] in EdgeIndex order."""
    assert ops and not ops & ~(OP_CHAINS | OP_CONNECT)
    g = StableGraph(n_vertices, edges, vertex_absent, edge_absent)
    census = set()
    vertex_state = [0 if there else ABSENT for there in g.node]
    edge_state = [0 if e is not None else ABSENT for e in g.edge]
    edge_chain = [NONE] * len(edges)
    n_chains = n_chains_removed = 0
    if ops & OP_CHAINS:                                                    # A:1044-1047
        chains, gone, removed_edges, orphans = prune_low_weight_chains(g, prune_factor, census)
        n_chains, n_chains_removed = len(chains), len(gone)
        for _, chain_edges in chains:
            for e in chain_edges:
                assert edge_chain[e] == NONE, "an edge in two chains"
                edge_chain[e] = chain_edges[0]
        for e in removed_edges:
            edge_state[e] |= REMOVED_CHAINS
        for v in orphans:
            vertex_state[v] |= REMOVED_CHAINS
        census.update(name for name, hit in (("chain removed", gone), ("chain kept", len(gone) < len(chains)), ("orphan removed", orphans),
                                             ("an edge in no chain", any(edge_chain[e] == NONE for e in range(len(edges)) if not edge_state[e] & ABSENT)),
                                             ("orphan kept: the only vertex", not orphans and g.count == 1 and not any(e is not None for e in g.edge)),
                                             ("a reference edge protects a low chain", any(all(g.pruning_multiplicity[e] < prune_factor for e in c[1]) and c not in gone for c in chains)))
                      if hit)
    flags = HAS_CYCLE if has_cycles(g) else 0                              # A:1056
    source, sink = get_reference_source_vertex(g), get_reference_sink_vertex(g)
    if source is None or sink is None:
        flags |= NO_REF_ENDS
    for v in dangling_tails(g):
        vertex_state[v] |= DANGLING_TAIL
    for v in dangling_heads(g):
        vertex_state[v] |= DANGLING_HEAD
    census.update(name for name, hit in (("cycle", flags & HAS_CYCLE), ("no ref ends", flags & NO_REF_ENDS), ("dangling tail", dangling_tails(g)),
                                         ("dangling head", dangling_heads(g)),
                                         ("one node: source and sink", source is not None and source == sink)) if hit)
    if ops & OP_CONNECT and not flags & NO_REF_ENDS:                       # A:1134
        vertices, removed_edges = remove_paths_not_connected_to_ref(g)
        for v in vertices:
            vertex_state[v] |= REMOVED_CONNECT
        for e in removed_edges:
            edge_state[e] |= REMOVED_CONNECT
        if vertices:
            census.add("connect removes")
    return dict(graph_flags=flags, n_chains=n_chains, n_chains_removed=n_chains_removed, n_vertices_left=len(g.node_indices()),
                n_edges_left=sum(e is not None for e in g.edge), ref_source=NONE if source is None else source,
                ref_sink=NONE if sink is None else sink, edge_chain=edge_chain, edge_state=edge_state, vertex_state=vertex_state, census=census)
