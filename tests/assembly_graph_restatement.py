"""A SERIAL, statement-by-statement Python restatement of the raw read-threading graph as build_graph_if_necessary leaves it,
next to the reference's line numbers: R = src/read_threading/read_threading_graph.rs, A = src/read_threading/
read_threading_assembler.rs, E = src/graphs/multi_sample_edge.rs.  It extends tests/assembly_kmers_restatement.py by import:
that file threads vertices and edges already; added here are the in-edge lists, increase_counts_in_matched_kmers with both
settings of increase_counts_through_branches, MultiSampleEdge's heap exactly as written (the push at creation, the pop at
capacity + 1, the peek), the flush behind every sample group, and reference_path.  It threads in the reference's order, one
sequence after the other, and looks at the graph "so far" where the reference does: what phmm_assembly_graph computes on the
device without any order is compared with this (tests/test_assembly_graph_hip.py), and the two share no shortcut.

Kmer equality is restated as equality of the bytes, as in assembly_kmers_restatement.py."""
import heapq
from collections import OrderedDict

import assembly_kmers_restatement as KR
from assembly_kmers_restatement import REF_SAMPLE, REF_SHORT, REF_NON_UNIQUE, LOW_COMPLEXITY, SequenceForKmers, kmer  # noqa: F401

TRACKED, REF_SOURCE = 1, 2
NO_VERTEX = 0xFFFFFFFF


class MultiSampleEdge:
    def __init__(self, is_ref, multiplicity, single_sample_capacity):      # E:119-131
        self.single_sample_multiplicities = []                             # BinaryHeap<Reverse<usize>>: a min-heap
        heapq.heappush(self.single_sample_multiplicities, multiplicity)    # E:121
        self.multiplicity = multiplicity
        self.is_ref = is_ref
        self.single_sample_capacity = single_sample_capacity
        self.current_single_sample_multiplicity = multiplicity
        self.popped = False                                                # (this file) census

    def flush_single_sample_multiplicity(self):                            # E:73-87
        heapq.heappush(self.single_sample_multiplicities, self.current_single_sample_multiplicity)
        if len(self.single_sample_multiplicities) == self.single_sample_capacity + 1:
            heapq.heappop(self.single_sample_multiplicities)               # remove the lowest multiplicity from the list
            self.popped = True
        elif len(self.single_sample_multiplicities) > self.single_sample_capacity + 1:
            raise AssertionError("Somehow the per sample multiplicity list has grown too big")
        self.current_single_sample_multiplicity = 0

    def inc_multiplicity(self, incr):                                      # E:89-92, the inherent method: Rust picks it over BaseEdge's
        self.multiplicity += incr
        self.current_single_sample_multiplicity += incr

    def get_pruning_multiplicity(self):                                    # E:94-96
        return self.single_sample_multiplicities[0]


class ReadThreadingGraph(KR.ReadThreadingGraph):
    INCREASE_COUNTS_BACKWARDS = True                                       # R: const

    def __init__(self, kmer_size, min_base_quality_to_use_in_assembly=10, num_pruning_samples=1):
        super().__init__(kmer_size, min_base_quality_to_use_in_assembly)
        self.num_pruning_samples = num_pruning_samples
        self.increase_counts_through_branches = False
        # base_graph: a vertex is its index; edge e is edge_source[e] -> edge_target[e] with weight[e]
        self.edge_source, self.edge_target, self.weight = [], [], []
        self.incoming = []          # per vertex, its in-edges in insertion order
        # (this file) what the outputs report
        self.creator = []           # per vertex: (owner, position) of the occurrence that created it
        self.lands = {}             # (owner, position) -> the vertex thread_sequence found or created there
        self.census = set()
        self._at = None

    def set_increase_counts_through_branches(self, value):
        self.increase_counts_through_branches = value

    def in_degree_of(self, vertex):
        return len(self.incoming[vertex])

    def create_vertex(self, sequence, k):                                  # R:626-632
        node_index = super().create_vertex(sequence, k)
        self.incoming.append([])
        self.creator.append(self._at)
        return node_index

    def add_edge(self, source, target, weight):                            # petgraph add_edge: indices in insertion order
        self.edge_source.append(source)
        self.edge_target.append(target)
        self.weight.append(weight)
        e = len(self.weight) - 1
        self.outgoing[source].append(e)
        self.incoming[target].append(e)
        self.edges.append([source, target, weight.is_ref, weight])         # (the base class's view, for chain())
        return e

    def build_graph_if_necessary(self, pending):                           # R:417-477
        if self.already_built:
            return
        self.preprocess_reads(pending)                                     # R:426
        for sequences_for_samples in pending.values():                     # R:430
            for sequence_for_kmers in sequences_for_samples:
                self.thread_sequence(sequence_for_kmers)                   # R:433
            for e in self.weight:                                          # R:454-456
                e.flush_single_sample_multiplicity()
        self.already_built = True                                          # R:472 (R:473-476: "+" on the vertices of the map)

    def thread_sequence(self, seq_for_kmers):                              # R:484-561
        start_pos = self.find_start(seq_for_kmers)                         # R:485
        if start_pos is None:
            self.census.add("no start")
            return
        self.starts.add((seq_for_kmers.owner, start_pos))
        if len(seq_for_kmers.sequence) <= start_pos + self.kmer_size:      # R:492
            self.census.add("sequence of k bases")
            return
        self._at = (seq_for_kmers.owner, start_pos)
        before = len(self.vertices)
        starting_vertex = self.get_or_create_kmer_vertex(seq_for_kmers.sequence, start_pos)   # R:496-497
        self.census.add("start: new vertex" if len(self.vertices) > before else "start: vertex of the map")
        self.visited.add((seq_for_kmers.owner, start_pos))
        self.lands[(seq_for_kmers.owner, start_pos)] = starting_vertex
        if self.INCREASE_COUNTS_BACKWARDS:                                 # R:499-507
            offset = self.kmer_size - 2 if self.kmer_size >= 2 else None   # checked_sub(2)
            if start_pos > 0 and offset is not None:
                self.census.add("walk from a start above 0")
            self.increase_counts_in_matched_kmers(seq_for_kmers, starting_vertex, seq_for_kmers.sequence, offset)
        if seq_for_kmers.is_ref:                                           # R:518-534
            assert self.ref_source is None, "Found two ref_sources!"
            self.reference_path = [starting_vertex]                        # R:525-528
            self.ref_source = kmer(seq_for_kmers.sequence, seq_for_kmers.start, self.kmer_size)
        vertex = starting_vertex                                           # R:536
        for i in range(start_pos + 1, seq_for_kmers.stop - self.kmer_size + 1):   # R:538
            self._at = (seq_for_kmers.owner, i)
            vertex = self.extend_chain_by_one(vertex, seq_for_kmers.sequence, i, seq_for_kmers.count, seq_for_kmers.is_ref)
            self.visited.add((seq_for_kmers.owner, i))
            self.lands[(seq_for_kmers.owner, i)] = vertex
            if seq_for_kmers.is_ref:                                       # R:546-548
                self.reference_path.append(vertex)

    def increase_counts_in_matched_kmers(self, seqs_for_kmers, vertex, original_kmer, offset):   # R:641-687
        if offset is None:                                                 # R:649
            self.census.add("walk: no offset")
            return
        for edge in reversed(list(self.incoming[vertex])):                 # R:651-658 (petgraph walks an adjacency list newest first)
            prev = self.edge_source[edge]                                  # R:659
            suffix = self.vertices[prev][-1]                               # R:660-665
            seq_base = original_kmer[offset]                               # R:666: the WHOLE sequence's byte at offset
            if suffix == seq_base and (self.increase_counts_through_branches or self.in_degree_of(vertex) == 1):   # R:668-671
                self.weight[edge].inc_multiplicity(seqs_for_kmers.count)   # R:672-676
                self.census.add("walk: step")
                if offset == 0:
                    self.census.add("walk: all k - 1 steps")
                self.increase_counts_in_matched_kmers(seqs_for_kmers, prev, original_kmer, offset - 1 if offset >= 1 else None)   # R:677-682
            elif suffix != seq_base:
                self.census.add("walk: suffix differs")
            else:
                self.census.add("walk: more than one in-edge")

    def extend_chain_by_one(self, prev_vertex, sequence, kmer_start, count, is_ref):   # R:700-769
        next_pos = kmer_start + self.kmer_size - 1                         # R:712
        for e in reversed(self.outgoing[prev_vertex]):                     # R:715-736
            target = self.edge_target[e]
            if self.vertices[target][-1] == sequence[next_pos]:            # get_suffix
                self.weight[e].inc_multiplicity(count)                     # R:738-747
                self.census.add("extend: edge followed")
                return target
        k = kmer(sequence, kmer_start, self.kmer_size)                     # R:750-751
        merge_vertex = self.get_next_kmer_vertex_for_chain_extension(k, is_ref, prev_vertex)   # R:752-753
        if merge_vertex is None:                                           # R:755-759
            next_vertex = self.create_vertex(sequence, k)
            self.census.add("extend: new vertex, " + ("non-unique" if k in self.non_unique_kmers else
                                                       "the reference source again" if k == self.ref_source else "unique"))
        else:
            next_vertex = merge_vertex
            self.census.add("extend: merged into the map's vertex")
        self.add_edge(prev_vertex, next_vertex, MultiSampleEdge(is_ref, count, self.num_pruning_samples))   # R:761-765
        return next_vertex

    def has_cycles(self):                                                  # base_graph: a directed cycle (Kahn)
        indeg = [len(i) for i in self.incoming]
        ready = [v for v, d in enumerate(indeg) if d == 0]
        seen = 0
        while ready:
            v = ready.pop()
            seen += 1
            for e in self.outgoing[v]:
                t = self.edge_target[e]
                indeg[t] -= 1
                if indeg[t] == 0:
                    ready.append(t)
        return seen != len(self.vertices)


def create_graph(reference, reads, kmer_size, min_base_quality=10, samples=None, num_pruning_samples=1):
    """A:924-1020 up to build_graph_if_necessary, with the default modes.  reads: (bases, quals) pairs of bytes; samples: a value
    per read.  Returns (status flags, graph): the graph is None for a reference shorter than k (A:935-938)."""
    if len(reference) < kmer_size:                                         # A:935-938
        return REF_SHORT, None
    flags = 0
    if KR.determine_non_unique_kmers(SequenceForKmers("ref", reference, 0, len(reference), 1, True, None), kmer_size):   # A:940-956
        flags |= REF_NON_UNIQUE
    rt_graph = ReadThreadingGraph(kmer_size, min_base_quality, num_pruning_samples)   # A:958-967
    rt_graph.set_threading_start_only_at_existing_vertex(False)           # A:980 with dangling-branch recovery on
    pending = OrderedDict()                                                # A:983 LinkedHashMap
    rt_graph.add_sequence(pending, "ref", REF_SAMPLE, reference, 0, len(reference), 1, True)   # A:984-994
    count = [0]                                                            # A:1004
    for r, (bases, quals) in enumerate(reads):                             # A:1008-1016
        rt_graph.add_read(bases, quals, samples[r] if samples is not None else 0, count, pending, r)
    rt_graph.build_graph_if_necessary(pending)                             # A:1020
    if rt_graph.is_low_quality_graph():
        flags |= LOW_COMPLEXITY
    rt_graph.group_order = [s for s in pending if s != REF_SAMPLE]         # (this file) census
    return flags, rt_graph


def graph(reference, reads, kmer_size, min_base_quality=10, samples=None, num_pruning_samples=1):
    """One (k, region) as phmm_assembly_graph reports it: flags; vertices [(seq, pos, flags)] in NodeIndex order; edges [(src,
    dst, is_ref, multiplicity, pruning multiplicity)] in EdgeIndex order; ref_path; ref_vertex and read_vertex[r] per position."""
    flags, g = create_graph(reference, reads, kmer_size, min_base_quality, samples, num_pruning_samples)
    out = dict(flags=flags, vertices=[], edges=[], ref_path=[], ref_vertex=[NO_VERTEX] * len(reference),
               read_vertex=[[NO_VERTEX] * len(b) for b, _ in reads], census=set(), group_order=[])
    if g is None:
        return out
    tracked = set(g.kmer_to_vertex_map.values())
    source = g.reference_path[0] if g.reference_path else None
    for v, (owner, pos) in enumerate(g.creator):
        out["vertices"].append((0 if owner is None else 1 + owner, pos, (TRACKED if v in tracked else 0) | (REF_SOURCE if v == source else 0)))
    for e, w in enumerate(g.weight):
        out["edges"].append((g.edge_source[e], g.edge_target[e], int(w.is_ref), w.multiplicity, w.get_pruning_multiplicity()))
        if w.popped:
            g.census.add("heap: popped")
    out["ref_path"] = list(g.reference_path)
    for (owner, pos), v in g.lands.items():
        (out["ref_vertex"] if owner is None else out["read_vertex"][owner])[pos] = v
    out["census"], out["group_order"] = g.census, g.group_order
    return out
