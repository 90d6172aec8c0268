"""A SERIAL restatement of the reference's dangling-end recovery -- recover_dangling_tails, then recover_dangling_heads
(read_threading_assembler.rs:1118-1131) -- statement by statement beside the reference's lines: R =
src/read_threading/read_threading_graph.rs, T = src/read_threading/abstract_read_threading_graph.rs, B = src/graphs/base_graph.rs,
U = src/reads/alignment_utils.rs, E = src/graphs/multi_sample_edge.rs.  It stands on the StableGraph model of
tests/assembly_prune_restatement.py (edges_directed newest first), aligns with the CPU oracle's Smith-Waterman and processes one
end after the other on the graph the ends before it left: nothing of how phmm_assembly_recover shares the work out is in here.
recover_all_dangling_branches = false only (give_up_at_branch = true in both find_path_* functions)."""
import assembly_prune_restatement as P
from oracle import oracle

OP_TAILS, OP_HEADS = 1, 2
TAIL, HEAD = 0, 1
(NO_PATH, LOOP, AT_REF_END, TOO_SHORT, CIGAR_NOT_OKAY, TOO_FEW_MATCHING, WHOLE_INSERTION, TOO_MANY_MISMATCHES, CANNOT_PUSH_REF,
 CANNOT_EXTEND, MERGED, NO_MERGE_POINT, REFERENCE_FAILS) = range(13)
STATUS_NAMES = ("no path", "loop", "at the reference end", "too short", "cigar not okay", "too few matching bases",
                "whole tail an insertion", "too many mismatches", "cannot push the reference back", "cannot extend", "merged",
                "no merge point", "the reference fails")
MAX_CIGAR_COMPLEXITY = 3                                                   # R:69
NONE = 0xFFFFFFFF
OP_M, OP_I, OP_D = 0, 1, 2
STANDARD_NGS = (25, -50, -110, -6)                                         # smith_waterman_aligner.rs:13


class Config:
    def __init__(self, ops=OP_TAILS | OP_HEADS, min_dangling_branch_length=4, min_matching_bases=-1, max_mismatches_in_dangling_head=-1,
                 num_pruning_samples=1, sw=STANDARD_NGS):
        self.ops, self.min_dangling_branch_length, self.min_matching_bases = ops, min_dangling_branch_length, min_matching_bases
        self.max_mismatches_in_dangling_head, self.num_pruning_samples, self.sw = max_mismatches_in_dangling_head, num_pruning_samples, tuple(sw)

    def key(self):
        return (self.ops, self.min_dangling_branch_length, self.min_matching_bases, self.max_mismatches_in_dangling_head, self.num_pruning_samples, self.sw)


class Graph(P.StableGraph):
    """the prune restatement's StableGraph with what recovery needs on top: the vertices' bytes, the edges' multiplicity, and
    add_node / add_edge (petgraph puts a new edge at the head of both lists: it is the newest).  The reuse of vacant slots by
    petgraph's add_edge is not modelled: a new element takes the next index."""

    def __init__(self, k, kmers, edges, vertex_absent=None, edge_absent=None):
        super().__init__(len(kmers), [(a, b, r, pm) for a, b, r, _, pm in edges], vertex_absent, edge_absent)
        self.k, self.kmers, self.multiplicity = k, [bytes(x) for x in kmers], [int(e[3]) for e in edges]

    def add_node(self, kmer):
        self.node.append(True)
        self.count += 1
        self.outgoing.append([])
        self.incoming.append([])
        self.kmers.append(bytes(kmer))
        return len(self.node) - 1

    def add_edge(self, a, b, is_ref, multiplicity, num_pruning_samples):   # E:119-131: the heap holds the one count
        self.edge.append((a, b))
        self.is_ref.append(bool(is_ref))
        self.multiplicity.append(multiplicity)
        self.pruning_multiplicity.append(multiplicity)                     # E:94-96, peek of a heap of one
        self.outgoing[a].append(len(self.edge) - 1)
        self.incoming[b].append(len(self.edge) - 1)
        return len(self.edge) - 1


def is_reference_node(g, v):                                               # B:130-146
    if any(g.is_ref[e] for e in g.edges_directed(v, False)) or any(g.is_ref[e] for e in g.edges_directed(v, True)):
        return True
    return g.count == 1


def get_next_reference_vertex(g, v, allow_non_ref_paths, blacklisted_edge):   # B:437-481
    for e in g.edges_directed(v, True):                                    # B:450-454: the newest reference edge
        if g.is_ref[e]:
            return g.edge_endpoints(e)[1]
    if not allow_non_ref_paths:
        return None
    edges = [e for e in g.edges_directed(v, True) if e != blacklisted_edge]   # B:461-474
    return g.edge_endpoints(edges[0])[1] if len(edges) == 1 else None      # B:476-480


def get_prev_reference_vertex(g, v):                                       # B:488-499
    return next((g.edge_endpoints(e)[0] for e in g.edges_directed(v, False) if is_reference_node(g, g.edge_endpoints(e)[0])), None)


def get_heaviest_edge(g, v, out):                                          # R:1703-1726: max_by keeps the LAST of equals
    edges = g.edges_directed(v, out)
    if len(edges) == 1:
        return edges[0]
    best = edges[0]
    for e in edges[1:]:
        if g.multiplicity[e] >= g.multiplicity[best]:
            best = e
    return best


class Fails(Exception):
    """the reference panics or never returns"""


def find_path(g, vertex, prune_factor, done, return_path, next_edge, next_node):   # R:1651-1692
    path, visited_nodes = [], set()
    v = vertex
    steps = 0
    while not done(v):
        edge = next_edge(v)
        if g.pruning_multiplicity[edge] < prune_factor:                    # R:1667-1677
            visited_nodes.update(path)
            path = []
        else:
            path.insert(0, v)                                              # R:1679
        v = next_node(edge)
        if v in path or v in visited_nodes:                                # R:1684-1687
            return LOOP, None
        steps += 1
        if steps > len(g.node):                                            # (a ring of low edges: the reference rides forever)
            raise Fails()
    path.insert(0, v)                                                      # R:1689
    return (None, path) if return_path(v) else (NO_PATH, None)             # R:1691


def find_path_upwards_to_lowest_common_ancestor(g, vertex, prune_factor):  # R:1595-1614
    return find_path(g, vertex, prune_factor,
                     lambda v: P.in_degree_of(g, v) != 1 or P.out_degree_of(g, v) >= 2,
                     lambda v: P.out_degree_of(g, v) > 1,
                     lambda v: g.edges_directed(v, False)[0], lambda e: g.edge_endpoints(e)[0])


def find_path_downwards_to_highest_common_descendant_of_reference(g, vertex, prune_factor):   # R:1505-1524
    return find_path(g, vertex, prune_factor,
                     lambda v: is_reference_node(g, v) or P.out_degree_of(g, v) != 1,
                     lambda v: is_reference_node(g, v),
                     lambda v: g.edges_directed(v, True)[0], lambda e: g.edge_endpoints(e)[1])


def get_reference_path(g, start, downwards, blacklisted_edge):             # R:1556-1577
    path, v = [], start
    while v is not None:
        if len(path) > len(g.node):                                        # (a cycle: the reference never returns)
            raise Fails()
        path.append(v)
        v = get_next_reference_vertex(g, v, True, blacklisted_edge) if downwards else get_prev_reference_vertex(g, v)
    return path


def get_bases_for_path(g, path, expand_source):                            # R:1735-1766
    return b"".join(g.kmers[v][::-1] if expand_source and P.in_degree_of(g, v) == 0 else g.kmers[v][-1:] for v in path)


def remove_trailing_deletions(cigar):                                      # U:702-707
    return cigar[:-1] if cigar[-1][0] == OP_D else cigar


def cigar_is_okay_to_merge(cigar, require_first_element_m, require_last_element_m):   # T:91-125
    if len(cigar) == 0 or len(cigar) > MAX_CIGAR_COMPLEXITY:
        return False
    if require_first_element_m and cigar[0][0] != OP_M:
        return False
    if require_last_element_m and cigar[-1][0] != OP_M:
        return False
    return True


def longest_suffix_match(seq, kmer, seq_start):                            # T:202-212
    for length in range(1, len(kmer) + 1):
        seq_i, kmer_i = seq_start - length + 1, len(kmer) - length
        if seq_i < 0 or seq[seq_i] != kmer[kmer_i]:
            return length - 1
    return len(kmer)


def ref_length(cigar):
    return sum(n for op, n in cigar if op in (OP_M, OP_D))


def read_length(cigar):
    return sum(n for op, n in cigar if op in (OP_M, OP_I))


def align(ref_bases, alt_bases, cfg):                                      # R:1408-1421, R:1471-1484
    elements, _ = oracle.sw_align(ref_bases, alt_bases, cfg.sw, "LeadingInDel")
    return remove_trailing_deletions([(int(e) & 15, int(e) >> 4) for e in elements])


def recover_dangling_tail(g, vertex, prune_factor, cfg, rec, new_edges):   # R:871-905, R:1370-1423
    min_tail_path_length = max(1, cfg.min_dangling_branch_length)          # R:1378
    status, alt_path = find_path_upwards_to_lowest_common_ancestor(g, vertex, prune_factor)   # R:1381-1382
    if alt_path is None:
        return status
    if P.is_ref_source(g, alt_path[0]):                                    # R:1386
        return AT_REF_END
    if len(alt_path) < min_tail_path_length + 1:                           # R:1387
        return TOO_SHORT
    ref_path = get_reference_path(g, alt_path[0], True, get_heaviest_edge(g, alt_path[1], False))   # R:1396-1400
    ref_bases, alt_bases = get_bases_for_path(g, ref_path, False), get_bases_for_path(g, alt_path, False)   # R:1403-1404
    cigar = align(ref_bases, alt_bases, cfg)
    rec.update(alt_len=len(alt_bases), ref_len=len(ref_bases), cigar=cigar)
    if not cigar_is_okay_to_merge(cigar, False, True):                     # R:898
        return CIGAR_NOT_OKAY
    # merge_dangling_tail, R:961-1036
    last_ref_index = ref_length(cigar) - 1                                 # R:976-977
    matching_suffix = min(longest_suffix_match(ref_bases, alt_bases, last_ref_index), cigar[-1][1])   # R:978-985
    if cfg.min_matching_bases >= 0:                                        # R:987-993
        if matching_suffix < cfg.min_matching_bases:
            return TOO_FEW_MATCHING
    elif matching_suffix == 0:
        return TOO_FEW_MATCHING
    alt_index_to_merge = max(max(read_length(cigar) - matching_suffix, 0) - 1, 0)   # R:995-1000
    first_element_is_deletion = cigar[0][0] == OP_D                        # R:1006-1009
    must_handle_leading_deletion_case = first_element_is_deletion and cigar[0][1] + matching_suffix == last_ref_index + 1   # R:1011-1013
    ref_index_to_merge = last_ref_index - matching_suffix + 1 + (1 if must_handle_leading_deletion_case else 0)   # R:1014-1020
    if ref_index_to_merge <= 0:                                            # R:1024-1026
        return WHOLE_INSERTION
    if ref_index_to_merge >= len(ref_path):                                # (R:1031 indexes past the path: a panic)
        return REFERENCE_FAILS
    e = g.add_edge(alt_path[alt_index_to_merge], ref_path[ref_index_to_merge], False, 1, cfg.num_pruning_samples)   # R:1029-1033
    rec["edge"] = len(new_edges)
    new_edges.append(e)
    return MERGED


def get_max_mismatches_legacy(g, cfg, length_of_dangling_branch):          # R:1142-1151
    return cfg.max_mismatches_in_dangling_head if cfg.max_mismatches_in_dangling_head > 0 else max(1, length_of_dangling_branch // g.k)


def best_prefix_match_legacy(g, cfg, path1, path2, max_index):             # R:1106-1131
    max_mismatches = get_max_mismatches_legacy(g, cfg, max_index)
    mismatches, last_good_index = 0, None
    for index in range(max_index):
        if path1[index] != path2[index]:
            mismatches += 1
            if mismatches > max_mismatches:
                return TOO_MANY_MISMATCHES, None
            last_good_index = index
    return NO_MERGE_POINT, last_good_index


def best_prefix_match(cfg, cigar, path1, path2):                           # R:1303-1351
    ref_idx, read_idx = ref_length(cigar) - 1, len(path2) - 1
    stop = False
    for op, n in reversed(cigar):                                          # R:1326-1343
        if op != OP_M:
            break
        for _ in range(n):
            if path1[ref_idx] != path2[read_idx]:
                stop = True
                break
            ref_idx -= 1
            read_idx -= 1
            if ref_idx < 0 or read_idx < 0:
                stop = True
                break
        if stop:
            break
    matches = len(path2) - 1 - read_idx                                    # R:1345
    return (-1, -1, True) if matches < cfg.min_matching_bases else (ref_idx, read_idx, False)


def extend_dangling_path_against_reference(g, cfg, cigar, dangling_path, reference_path, num_nodes_to_extend, new_edges, new_vertices, removed):   # R:1209-1291
    index_of_last_dangling_node = len(dangling_path) - 1
    offset_for_ref_end_to_dangling_end = ref_length(cigar) - read_length(cigar)   # R:1215-1234
    index_of_ref_node_to_use = index_of_last_dangling_node + offset_for_ref_end_to_dangling_end + num_nodes_to_extend
    if index_of_ref_node_to_use >= len(reference_path) or index_of_ref_node_to_use < 0:   # R:1240-1244
        return False
    dangling_source = dangling_path.pop(index_of_last_dangling_node)       # R:1246-1248
    ref_source_sequence = g.kmers[reference_path[index_of_ref_node_to_use]]
    sequence_to_extend = ref_source_sequence[:num_nodes_to_extend] + g.kmers[dangling_source]   # R:1258-1268
    source_edge = get_heaviest_edge(g, dangling_source, True)              # R:1272
    prev_v = g.edge_endpoints(source_edge)[1]
    multiplicity = g.multiplicity[source_edge]
    g.remove_edge(source_edge)                                             # R:1274
    removed.append(source_edge)
    for i in range(num_nodes_to_extend, 0, -1):                            # R:1278-1288
        new_v = g.add_node(sequence_to_extend[i:i + g.k])
        new_vertices.append(new_v)
        new_edges.append(g.add_edge(new_v, prev_v, False, multiplicity, cfg.num_pruning_samples))
        dangling_path.append(new_v)
        prev_v = new_v
    return True


def recover_dangling_head(g, vertex, prune_factor, cfg, rec, new_edges, new_vertices, removed):   # R:917-953, R:1435-1486
    status, alt_path = find_path_downwards_to_highest_common_descendant_of_reference(g, vertex, prune_factor)   # R:1444-1448
    if alt_path is None:
        return status
    if P.is_ref_sink(g, alt_path[0]):                                      # R:1453
        return AT_REF_END
    if len(alt_path) < cfg.min_dangling_branch_length + 1:                 # R:1454
        return TOO_SHORT
    ref_path = get_reference_path(g, alt_path[0], False, None)             # R:1463
    ref_bases, alt_bases = get_bases_for_path(g, ref_path, True), get_bases_for_path(g, alt_path, True)   # R:1466-1467
    cigar = align(ref_bases, alt_bases, cfg)
    rec.update(alt_len=len(alt_bases), ref_len=len(ref_bases), cigar=cigar)
    if not cigar_is_okay_to_merge(cigar, True, False):                     # R:944
        return CIGAR_NOT_OKAY
    if cfg.min_matching_bases >= 0:                                        # R:946-947, merge_dangling_head R:1159-1207
        i0, i1, few = best_prefix_match(cfg, cigar, ref_bases, alt_bases)
        if few:
            return TOO_FEW_MATCHING
        if i0 <= 0 or i1 <= 0:                                             # R:1179-1181
            return NO_MERGE_POINT
        if i0 >= len(ref_path) - 1:                                        # R:1184-1186
            return CANNOT_PUSH_REF
    else:                                                                  # merge_dangling_head_legacy R:1044-1095
        why, i0 = best_prefix_match_legacy(g, cfg, ref_bases, alt_bases, cigar[0][1])   # R:1058-1062
        if i0 is None:
            return why
        i1 = i0
        if i0 >= len(ref_path) - 1:                                        # R:1068-1070
            return CANNOT_PUSH_REF
    num_nodes_to_extend = i1 - len(alt_path) + 2                           # R:1189-1190, R:1073-1074
    if i1 >= len(alt_path) and not extend_dangling_path_against_reference(g, cfg, cigar, alt_path, ref_path, num_nodes_to_extend, new_edges,
                                                                          new_vertices, removed):   # R:1191-1198, R:1076-1083
        return CANNOT_EXTEND
    e = g.add_edge(ref_path[i0 + 1], alt_path[i1], False, 1, cfg.num_pruning_samples)   # R:1200-1204, R:1086-1090
    rec["edge"] = len(new_edges)
    new_edges.append(e)
    return MERGED


def recover(k, kmers, edges, prune_factor, cfg, vertex_absent=None, edge_absent=None):
    """One graph as phmm_assembly_recover reports it.  kmers: the vertices' bytes in NodeIndex order; edges: [(source, target,
    is_ref, multiplicity, pruning multiplicity)] in EdgeIndex order."""
    g = Graph(k, kmers, edges, vertex_absent, edge_absent)
    n_vertices, n_edges = len(kmers), len(edges)
    ends, new_edges, new_vertices, removed = [], [], [], []
    counts = dict(n_tails=0, n_tails_recovered=0, n_heads=0, n_heads_recovered=0)
    census = set()
    for kind in (TAIL, HEAD):
        if not cfg.ops & (OP_TAILS if kind == TAIL else OP_HEADS):
            continue
        todo = P.dangling_tails(g) if kind == TAIL else P.dangling_heads(g)   # R:792-797, R:837-842: listed before any is touched
        for v in todo:                                                     # R:801-811, R:847-857
            rec = dict(vertex=v, kind=kind, alt_len=0, ref_len=0, cigar=[], edge=NONE)
            n_v = len(new_vertices)
            try:
                rec["status"] = recover_dangling_tail(g, v, prune_factor, cfg, rec, new_edges) if kind == TAIL else \
                    recover_dangling_head(g, v, prune_factor, cfg, rec, new_edges, new_vertices, removed)
            except Fails:
                rec["status"] = REFERENCE_FAILS
            ends.append(rec)
            census.add(STATUS_NAMES[rec["status"]])
            if len(new_vertices) > n_v:
                census.add("extension")
            counts["n_tails" if kind == TAIL else "n_heads"] += 1
            counts["n_tails_recovered" if kind == TAIL else "n_heads_recovered"] += rec["status"] == MERGED
    out = dict(counts, n_new_edges=len(new_edges), n_new_vertices=len(new_vertices), census=census)
    out.update(end_vertex=[r["vertex"] for r in ends], end_kind=[r["kind"] for r in ends], end_status=[r["status"] for r in ends],
               end_alt_len=[r["alt_len"] for r in ends], end_ref_len=[r["ref_len"] for r in ends], end_n_cigar=[len(r["cigar"]) for r in ends],
               end_cigar=[[(n << 4) | op for op, n in r["cigar"][:4]] + [0] * (4 - min(4, len(r["cigar"]))) for r in ends],
               end_edge=[r["edge"] for r in ends])
    gone = lambda e: g.edge[e] is None  # noqa: E731  (a new edge that a later extension took out again: vacant)
    out.update(new_edge_src=[NONE if gone(e) else g.edge[e][0] for e in new_edges], new_edge_dst=[NONE if gone(e) else g.edge[e][1] for e in new_edges],
               new_edge_multiplicity=[g.multiplicity[e] for e in new_edges], new_edge_pruning_multiplicity=[g.pruning_multiplicity[e] for e in new_edges],
               new_vertex_kmer=[g.kmers[v] for v in new_vertices],
               edge_removed=[int(e in removed) for e in range(n_edges)])
    assert new_vertices == list(range(n_vertices, n_vertices + len(new_vertices)))
    assert new_edges == list(range(n_edges, n_edges + len(new_edges)))
    out["graph"] = g
    return out
